"""gmg_charge_density, gmg_get_charge_density and gmg_rhs_assemble on the MI355X (csrc/gmg_device.hpp: charge_density_kernel,
rhs_cell_kernel, rhs_terms_kernel, rhs_gather_kernel) through the C ABI on synthetic inputs, against the independent
references of tests/rhs_reference.py: densities within the bound derived there (mpmath on sampled outputs, numpy on all),
the right-hand side bit for bit against the header's arithmetic restated in numpy and within the bound against mpmath; and
the driver's cycle 0 on a gas against a right-hand side built from the DoF coordinates alone.  Each test prints its worst
error / bound (DESIGN.md section 11 quotes them)."""
import numpy as np
import pytest

import rhs_reference as rr
from gpu_util import capi
from test_rhs_reference_cpu import DENSITY_PARAMS, check_end_to_end, end_to_end_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi().Context(1)
    yield c
    c.close()


def device_density(ctx, G, use_lists, dens=True):
    return ctx.charge_density(G["cell_lo"], G["cell_h"], G["root_lo"], G["root_h"], G["x"], G["q"], G["r_c"], G["cutoff"], use_lists,
                              G["qp"], dens=dens)


@pytest.mark.parametrize("name,use_lists", DENSITY_PARAMS)
def test_charge_density(ctx, name, use_lists):
    R = rr.density_reference(name, use_lists)
    G = R["G"]
    rho = device_density(ctx, G, use_lists)
    rr.check_density("device", name, use_lists, R, rho)
    assert device_density(ctx, G, use_lists, dens=None) is None  # kept on the device: the same bits come back
    assert np.array_equal(ctx.get_charge_density(*rho.shape), rho)
    with pytest.raises(capi().GMGError) as e:
        ctx.get_charge_density(rho.shape[0] + 1, rho.shape[1])
    assert e.value.code == capi().ERR_INVALID


def test_membership_at_the_cutoff(ctx):
    """atoms on, one ulp inside and one ulp outside the cutoff sphere of each of the 8 root vertices, on and off an axis, and
    the tie of the vertex choice: each atom alone gives exactly 0 or its own addend; all together stay within the bound"""
    G, expect, _ = rr.edge_case()
    for k in range(len(expect)):
        one = dict(G, x=G["x"][k:k + 1], q=G["q"][k:k + 1])
        rho = device_density(ctx, one, True)
        assert bool(np.all(rho != 0.0)) == bool(expect[k]) and bool(np.all(rho == 0.0)) != bool(expect[k]), (k, G["x"][k], expect[k])
    idx = rr.sample(len(G["cell_h"]) * len(G["qp"]))
    ref = rr.density_numpy(G, True)
    assert np.all(ref["count"] == expect.sum())
    # (the mpmath tier with the fp64 membership of the header: the 8 atoms below the cutoff by less than fp64 resolves are off)
    keep = dict(G, x=G["x"][expect], q=G["q"][expect])
    refm = rr.density_mp(keep, False, idx)
    rho = device_density(ctx, G, True)
    r_np, r_mp = rr.ratio(rho - ref["rho"], 2.0 * ref["bound"]), rr.ratio(rho.reshape(-1)[idx] - refm["rho"], refm["bound"])
    print(f"device density at the cutoff: {expect.sum()} of {len(expect)} atoms on the list, error / bound {r_mp:.2e} (mpmath) {r_np:.2e} (numpy)")
    assert max(r_np, r_mp) <= 1.0


def assemble(ctx, T, dens_shape=None):
    n = len(T["dof_ptr"]) - 1
    out = ctx.vector(n)
    try:
        ctx.rhs_assemble(T["n_cells"], T["dim"], T["shape"], T["weight"], T["cell_level"], T["jxw"], T["term_slot"], T["term_value"],
                         T["dof_ptr"], T["entry_slot"], T["entry_coef"], T["coef_table"], out)
        return out.download()
    finally:
        out.free()


@pytest.mark.parametrize("name", list(rr.RHS_CASES))
def test_rhs_assemble(ctx, name):
    T = rr.rhs_tables(name)
    copied = device_density(ctx, T["geometry"], False)
    assert device_density(ctx, T["geometry"], False, dens=None) is None  # (a later call with a host array would drop them)
    dens = ctx.get_charge_density(T["n_cells"], T["nq"])
    assert np.array_equal(dens, copied)
    got = assemble(ctx, T)
    ref, _ = rr.rhs_numpy(dens, T)
    wrong = np.nonzero(got != ref)[0]
    assert len(wrong) == 0, (len(wrong), wrong[:5], got[wrong[:5]], ref[wrong[:5]])
    assert not np.signbit(got[np.diff(T["dof_ptr"]) == 0]).any()
    idx = rr.rhs_sample(T)
    m = rr.rhs_mp(dens, T, idx)
    r = rr.ratio(got[idx] - m["rhs"], m["bound"])
    print(f"device rhs {name}: all {len(got)} DoFs bit for bit; error / bound {r:.2e} (mpmath, {len(idx)} DoFs)")
    assert r <= 1.0


def test_rhs_assemble_refusals():
    """every GMG_ERR_INVALID of the header, found on the host; the context works after each"""
    C = capi()
    c = C.Context(1)
    T = rr.rhs_tables("d3-nq8")
    try:
        def refused(**change):
            with pytest.raises(C.GMGError) as e:
                assemble(c, dict(T, **change))
            assert e.value.code == C.ERR_INVALID, change.keys()

        refused()  # no gmg_charge_density(..., dens = NULL) before it
        device_density(c, T["geometry"], False)  # densities copied out do not stay either
        refused()
        device_density(c, T["geometry"], False, dens=None)
        dens = c.get_charge_density(T["n_cells"], T["nq"])
        ref, _ = rr.rhs_numpy(dens, T)
        n_slots = T["n_cells"] * 8

        def works():
            assert np.array_equal(assemble(c, T), ref)

        works()
        refused(n_cells=T["n_cells"] - 1)  # shape mismatch: cells
        works()
        refused(weight=T["weight"][:-1], shape=T["shape"][:-1])  # shape mismatch: nq
        works()
        refused(dim=2, shape=T["shape"][:, :4])  # slots beyond n_cells * 4
        works()
        for k, bad in ((5, n_slots), (len(T["entry_slot"]) - 1, -1)):
            es = T["entry_slot"].copy()
            es[k] = bad
            refused(entry_slot=es)
            works()
        for k, bad in ((len(T["term_slot"]) - 1, n_slots), (0, -1), (400, 0)):  # out of range, and not ascending
            ts = T["term_slot"].copy()
            ts[k] = bad
            refused(term_slot=ts)
            works()
        for k, bad in ((7, T["dof_ptr"][6] - 1), (0, -1)):
            ptr = T["dof_ptr"].copy()
            ptr[k] = bad
            refused(dof_ptr=ptr)
            works()
        lv = T["cell_level"].copy()
        lv[3] = 16
        refused(cell_level=lv)
        works()
        # nq = 513 is refused whatever is on the device; 512 is the largest that works (test_rhs_assemble)
        big = dict(T, nq=513, shape=np.zeros((513, 8)), weight=np.ones(513))
        G = dict(T["geometry"], qp=np.full((513, 3), 0.5))
        device_density(c, G, False, dens=None)
        with pytest.raises(C.GMGError) as e:
            assemble(c, big)
        assert e.value.code == C.ERR_INVALID
        device_density(c, T["geometry"], False, dens=None)
        works()
    finally:
        c.close()


@pytest.mark.parametrize("use_lists", [False, True])
@pytest.mark.parametrize("dens_dev,rhs_dev", [(True, True), (True, False), (False, False)])
def test_driver_rhs_from_a_gas(use_lists, dens_dev, rhs_dev):
    """cycle 0 of the driver with the device in use: densities and right-hand side on the device, densities alone, neither"""
    p, x, q = end_to_end_problem(use_lists, dens_dev, rhs_dev)
    p.run_cycle(0, on_device=True)
    check_end_to_end(f"driver, densities on device {int(dens_dev)}, rhs on device {int(rhs_dev)},", p, x, q, use_lists)
    p.close()
