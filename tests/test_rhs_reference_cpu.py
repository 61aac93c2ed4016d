"""The references of tests/rhs_reference.py checked where no GPU exists: the fp64 numpy tier against the mpmath tier on every
case the GPU tests run (tests/test_gpu_rhs_reference.py), the conditions on their inputs, and the host loop of the driver
(compute_charge_densities + assemble_system) against a right-hand side built from the DoF coordinates, the quadrature rule
and the atoms alone.  Each test prints its worst error / bound."""
import numpy as np
import pytest

import atoms_reference as ar
import rhs_reference as rr
from gpu_util import pkg

DENSITY_PARAMS = [(n, l) for n in rr.DENSITY_CASES for l in (0, 1)]


@pytest.mark.parametrize("name,use_lists", DENSITY_PARAMS)
def test_density_tiers_agree(name, use_lists):
    R = rr.density_reference(name, use_lists)
    G = R["G"]
    # a condition on the inputs, not a tolerance: no atom of a gas within 64 ulp of a cutoff sphere
    assert rr.cutoff_gap_ulps(G["root_lo"], G["root_h"], G["x"], G["cutoff"]) > rr.GAP_ULPS
    for ci in (0, len(G["cell_h"]) - 1):
        assert np.array_equal(rr.members_fp64(G["root_lo"][ci], G["root_h"], G["x"], G["cutoff"]),
                              rr.members_exact(G["root_lo"][ci], G["root_h"], G["x"], G["cutoff"]))
    rr.check_density("numpy tier", name, use_lists, R, R["np"]["rho"])
    if use_lists and len(G["x"]) >= 64:
        assert (R["np"]["count"] > 0).any()


def test_membership_edge_construction():
    """every atom of the edge case is where the docstring says, in fp64 and exactly"""
    G, expect, robust = rr.edge_case()
    rlo = G["root_lo"][0]
    fp = np.zeros(len(expect), bool)
    fp[rr.members_fp64(rlo, G["root_h"], G["x"], G["cutoff"])] = True
    ex = np.zeros(len(expect), bool)
    ex[rr.members_exact(rlo, G["root_h"], G["x"], G["cutoff"])] = True
    assert np.array_equal(fp, expect)
    assert np.array_equal(ex[robust], expect[robust])
    assert ex[~robust].all() and not fp[~robust].any() and (~robust).sum() == 8  # below the cutoff by less than fp64 resolves
    # an atom wrongly on or off a list changes rho by far more than the tolerance
    ref = rr.density_numpy(G, True)
    pts = rr.points(G["cell_lo"], G["cell_h"], G["qp"])
    d = G["x"][None, None, :, :] - pts[:, :, None, :]
    t = rr.constant(G["r_c"]) * np.exp(-(d * d).sum(-1) / G["r_c"] ** 2) * np.abs(G["q"])
    worst = (t.min(-1) / ref["bound"]).min()
    print(f"edge case: smallest single-atom addend / tolerance {worst:.3g}")
    assert worst >= 1000.0


@pytest.mark.parametrize("name", list(rr.RHS_CASES))
def test_rhs_tiers_agree(name):
    T = rr.rhs_tables(name)
    dens = rr.density_numpy(T["geometry"], False)["rho"]
    rhs, F = rr.rhs_numpy(dens, T)
    idx = rr.rhs_sample(T)
    m = rr.rhs_mp(dens, T, idx)
    r = rr.ratio(rhs[idx] - m["rhs"], m["bound"])
    cnt = np.diff(T["dof_ptr"])
    print(f"rhs {name}: numpy vs mpmath error / bound {r:.2e} ({len(idx)} DoFs of {len(cnt)}, {len(T['term_slot'])} terms)")
    assert r <= 1.0 and np.isfinite(rhs).all()
    assert np.all(rhs[cnt == 0] == 0.0)
    if name == "d3-nq8":
        assert set(cnt) >= {0, 1, 8, 40} and set(T["entry_coef"]) == set(range(256)) and set(T["cell_level"]) == set(range(16))
        runs = np.diff(np.nonzero(np.diff(T["term_slot"], prepend=-1, append=2 ** 30))[0])
        assert set(runs) == {1, 2, 300, 3000} and runs[0] == 300 and runs[-1] == 3000


E2E_ATOMS, E2E_RC, E2E_CUT = 40, 0.5, 3.5


def end_to_end_problem(use_lists, dens_dev=False, rhs_dev=False):
    S = pkg().step50
    pkg().build.build_all()
    p = S.Problem(S.prm_text(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Homogeneous", cycles=1,
                             r_c=E2E_RC, cutoff=E2E_CUT, rhs_optimization=bool(use_lists), quad_rhs=1, global_refinement=0,
                             smoother="Jacobi", densities_on_device=dens_dev, rhs_on_device=rhs_dev))
    x, q, _ = ar.gas(700, E2E_ATOMS, E2E_RC)
    p.set_atoms(q, x)
    return p, x, q


def check_end_to_end(what, p, x, q, use_lists):
    X, free = p.dof_coordinates(), ~p.constrained_mask()
    ref, bound, gap = rr.end_to_end_reference(X, x, q, E2E_RC, E2E_CUT * E2E_RC, 2, use_lists)
    assert gap > 1e-9  # a condition on the atoms: none next to a cutoff sphere, where host and device could differ
    got = p.vector("rhs")
    r = rr.ratio((got - ref)[free], 2.0 * bound[free])
    print(f"{what} lists {int(use_lists)}: rhs of {free.sum()} unconstrained DoFs, {(ref[free] != 0).sum()} nonzero, error / bound {r:.2e}")
    assert (ref[free] != 0).sum() > 500 and np.isfinite(got).all() and r <= 1.0
    return r


@pytest.mark.parametrize("use_lists", [False, True])
def test_host_rhs_from_a_gas(use_lists):
    p, x, q = end_to_end_problem(use_lists)
    p.run_cycle(0, on_device=False)
    check_end_to_end("host loop", p, x, q, use_lists)
    p.close()
