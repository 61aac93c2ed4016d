"""The atom-side kernels on the MI355X (csrc/gmg_forces.hpp: atom_field_kernel, pair_all_kernel, pair_binned_kernel;
csrc/gmg_exact.hpp: gauss_potential_kernel, energy_error_kernel) through the C ABI with synthetic inputs, against the
independent references of tests/atoms_reference.py: mpmath on sampled outputs, fp64 numpy on all, within the bound derived
there.  No Problem and no mesh of the driver.  Every case runs with force_block 64, 128 and 256 and must give the same bits;
each test prints its worst error / bound (DESIGN.md sections 9 and 10 quote them)."""
import math

import numpy as np
import pytest

import atoms_reference as ar
from gpu_util import capi

pytestmark = pytest.mark.gpu
BLOCKS = (64, 128, 256)


@pytest.fixture(scope="module")
def ctx():
    c = capi().Context(1)
    # the locator of a one-cell mesh with u = 0: no field, so F = F^s
    c.set_point_locator([1, 1, 1], [0.0, 0.0, 0.0], 1.0, np.array([-1], dtype=np.int32), np.arange(8, dtype=np.int32).reshape(1, 8))
    c.u0 = c.vector(8, np.zeros(8))
    yield c
    c.set_option("force_block", 64)
    c.set_option("exact_chunk_log2", 35)
    c.close()


def same_bits(runs):
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert np.array_equal(a, b), "the result depends on force_block"


@pytest.mark.parametrize("case_id", list(ar.PAIR_CASES))
def test_short_range_pair_sums(ctx, case_id):
    R = ar.pair_reference(case_id)
    ar.check_pair_inputs(case_id, R)
    runs = []
    for block in BLOCKS:
        ctx.set_option("force_block", block)
        out = ctx.atom_forces(R["x"], R["q"], ctx.u0, R["r_c"], R["cutoff"])
        assert not out["phi"].any() and not out["field"].any() and np.array_equal(out["force"], out["force_short"])
        runs.append((out["force_short"], out["e_short"]))
    same_bits(runs)
    ar.check_pair_outputs("device", case_id, R, *runs[0])


@pytest.mark.parametrize("case_id", list(ar.DIRECT_CASES))
def test_direct_coulomb(ctx, case_id):
    R = ar.pair_reference(case_id, law="direct")
    runs = []
    for block in BLOCKS:
        ctx.set_option("force_block", block)
        runs.append(ctx.direct_coulomb(R["x"], R["q"]))
    same_bits(runs)
    ar.check_pair_outputs("device direct", case_id, R, *runs[0])


@pytest.mark.parametrize("key", list(ar.POTENTIAL_CASES))
def test_exact_potential(ctx, key):
    R = ar.potential_reference(key)
    x, q, r_c, pts = R["x"], R["q"], R["r_c"], R["pts"]
    chunk = max(0, math.ceil(math.log2(ar.POINTS_PER_LAUNCH * len(q))))  # launch cuts between the sampled points
    assert ar.POINTS_PER_LAUNCH <= (1 << chunk) // len(q) < 2 * ar.POINTS_PER_LAUNCH + 2
    runs = []
    for block, log2 in [(b, chunk) for b in BLOCKS] + [(64, 35)]:
        ctx.set_option("force_block", block)
        ctx.set_option("exact_chunk_log2", log2)
        phi, grad = ctx.gaussian_potential(x, q, r_c, pts)
        only_phi, _ = ctx.gaussian_potential(x, q, r_c, pts, want_grad=False)
        _, only_grad = ctx.gaussian_potential(x, q, r_c, pts, want_phi=False)
        assert np.array_equal(only_phi, phi) and np.array_equal(only_grad, grad)  # the three template variants
        runs.append((phi, grad))
    ctx.set_option("exact_chunk_log2", 35)
    same_bits(runs)
    ar.check_potential_outputs("device", key, R, *runs[0])


@pytest.mark.parametrize("r_c", [0.5, 0.37])
@pytest.mark.parametrize("n_atoms", [1, 2])
def test_gradient_close_to_an_atom(ctx, r_c, n_atoms):
    """at 2e-10 ... 0.1 r_c from an atom its own contribution to grad phi is accurate to a few ulp of itself"""
    x, q, pts = ar.near_atom_case(r_c)
    x, q = x[:n_atoms], q[:n_atoms]
    runs = []
    for block in BLOCKS:
        ctx.set_option("force_block", block)
        runs.append(ctx.gaussian_potential(x, q, r_c, pts))
    same_bits(runs)
    ar.check_near_atom("device", r_c, x, q, pts, *runs[0])


@pytest.mark.parametrize("n1", [1, 2, 3, 4])
def test_error_norm(ctx, n1):
    """nq = 1, 8, 27, 64 quadrature points per cell: 64, 8, 2 (ten idle lanes) and 1 cells per workgroup of 64; 301 cells leave
    the last workgroup partly filled; exact_chunk_log2 = 11 with 40 atoms cuts a call into launches of 51 / nq cells, inside
    a workgroup's worth of them"""
    E = ar.error_norm_case()
    nc, nq = len(E["h"]), n1 ** 3
    sample = np.array(sorted({0, 1, 7, 8, 50, 51, 63, 64, 127, 128, nc - 2, nc - 1}))[:12 if nq < 64 else 6]
    if nq == 64:
        sample = np.append(sample[:5], nc - 1)
    ref = ar.error_norm_reference(E, n1, sample)
    u = ctx.vector(len(E["u"]), E["u"])
    runs = []
    try:
        for block, log2 in [(b, 11) for b in BLOCKS] + [(64, 35), (256, 13)]:
            ctx.set_option("force_block", block)
            ctx.set_option("exact_chunk_log2", log2)
            err, ce = ctx.energy_norm_error(E["lo"], E["h"], E["dofs"], u, E["x"], E["q"], E["r_c"], ref["qp"], ref["w"], ref["sg"])
            runs.append((ce, np.array([err])))
    finally:
        ctx.set_option("exact_chunk_log2", 35)
        u.free()
    same_bits(runs)
    ce, err = runs[0][0], float(runs[0][1][0])
    r_np, r_mp = ar.ratio(ce - ref["cell_err2"], ref["bound"]), ar.ratio(ce[sample] - ref["mp"], ref["bound_mp"])
    total = math.sqrt(math.fsum(ce))
    # the sum over the cells in any order is off by at most (n - 1) u of the non-negative total, the root halves that
    r_norm = abs(err - total) / ((nc / 2 + 1) * ar.U * total)
    print(f"device error norm nq {nq}: error / bound  cell_err2 {r_mp:.2e} (mpmath, {len(sample)} cells) {r_np:.2e} (numpy, all {nc})  "
          f"norm {r_norm:.2e}")
    assert np.all(ce > 0.0) and max(r_np, r_mp, r_norm) <= 1.0


def test_error_norm_refuses_more_than_64_points(ctx):
    C = capi()
    E = ar.error_norm_case()
    u = ctx.vector(len(E["u"]), E["u"])
    try:
        with pytest.raises(C.GMGError) as e:
            ctx.energy_norm_error(E["lo"], E["h"], E["dofs"], u, E["x"], E["q"], E["r_c"], np.full((65, 3), 0.5), np.full(65, 1.0 / 65),
                                  np.zeros((65, 8, 3)))
        assert e.value.code == C.ERR_UNSUPPORTED
    finally:
        u.free()


FORESTS = {
    # every plane origin + h c is exact in fp64 (h0 a power of two, |coordinates| < 2): a point placed on a face is on it
    # for the device's walk too, so faces, edges, vertices, the boundary and the outside are all tested
    "4x4x4-ties": dict(n0=(4, 4, 4), origin=(-1.3, -1.7, -1.1), h0=0.5, ties=True),
    # planes that round: random points only, none within 2^-10 of the smallest edge of a plane
    "3x2x1": dict(n0=(3, 2, 1), origin=(0.3, -1.7, 5.1), h0=0.7, ties=False),
}


@pytest.mark.parametrize("name", list(FORESTS))
def test_field_on_a_synthetic_forest(name):
    """gmg_set_point_locator + gmg_atom_forces (phi and E) on a forest refined at random to depth 4 without 2:1 balance,
    every cell with its own 8 DoFs of a random u: any wrong cell, level or octant changes the result by O(1)"""
    f = FORESTS[name]
    F = ar.Forest(6, f["n0"], f["origin"], f["h0"])
    assert set(F.cell_level) == {0, 1, 2, 3, 4}
    rng = np.random.default_rng(21)
    u = rng.normal(size=8 * F.n_active)
    pts = ar.forest_points(F, 10, ties=f["ties"])
    if not f["ties"]:
        pts = pts[F.face_distance(pts) > 2.0 ** -10 * F.h0 / 16]
        assert len(pts) > 250
    ref = ar.field_numpy(F, u, pts)
    if f["ties"]:
        assert set(ref["used"]) == {0, 1, 2, 4, 8} and (ref["used"] == 8).sum() > 500
    idx = np.arange(0, len(pts), 11)
    refm = ar.field_mp(F, u, pts, idx)
    ctx = capi().Context(1)
    runs = []
    try:
        ctx.set_point_locator(F.n0, F.origin, F.h0, F.node, F.active_dofs)
        du = ctx.vector(len(u), u)
        for block in BLOCKS:
            ctx.set_option("force_block", block)
            out = ctx.atom_forces(pts, np.ones(len(pts)), du, 0.5, 1.0)
            runs.append((out["phi"], out["field"]))
    finally:
        ctx.close()
    same_bits(runs)
    phi, E = runs[0]
    assert np.isfinite(phi).all() and np.isfinite(E).all()
    assert np.all(E[ref["used"] == 0] == 0.0)  # no octant left in the lattice: E = 0, phi the clamped cell's extrapolation
    rs = dict(phi_np=ar.ratio(phi - ref["phi"], ref["bound_phi"]), E_np=ar.ratio(E - ref["E"], ref["bound_E"]),
              phi_mp=ar.ratio(phi[idx] - refm["phi"], ref["bound_phi"][idx]), E_mp=ar.ratio(E[idx] - refm["E"], ref["bound_E"][idx]))
    print(f"device field {name}: {F.n_active} cells, {len(pts)} points, error / bound  phi {rs['phi_mp']:.2e} E {rs['E_mp']:.2e} "
          f"(mpmath, {len(idx)} points)  phi {rs['phi_np']:.2e} E {rs['E_np']:.2e} (numpy, all)")
    assert max(rs.values()) <= 1.0, rs
