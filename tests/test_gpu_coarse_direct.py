"""The direct coarse solver on the level-0 lattice (csrc/gmg_fastdiag.hpp) against
tests/fastdiag_reference.py: every pass of every shape within the componentwise bound of a product of m terms, the lane map
of the f64 matrix instruction with unit vectors, the solve within the two bounds derived from the reference's kappa_2,
determinism, the refusals, whole adaptive runs with and without the prm key, and the life cycle of its allocations.
The shapes, vectors and bounds are those tests/test_fastdiag_reference_cpu.py proves the numpy restatement against."""
from types import SimpleNamespace

import numpy as np
import pytest

import fastdiag_reference as F
from gpu_util import capi, pkg

pytestmark = pytest.mark.gpu

SHAPE_IDS = [F.shape_id(s) for s in F.SHAPES]
LANE_SHAPES = [(19, 6, 35), (35, 19, 6), (6, 35, 19)]


def direct_context(shape, Ke=None):
    C = capi()
    c = C.Context(1)
    c.set_level_matrix_lattice(0, shape, F.cell_matrix() if Ke is None else Ke)
    c.set_coarse_solver(C.COARSE_DIRECT)
    return c


def solve(c, b, want_residual=True):
    vb, vx = c.vector(len(b), b), c.vector(len(b), np.full(len(b), np.nan))
    it, res, rc = c.coarse_solve(vx, vb, want_residual)
    x = vx.download()
    vb.free(); vx.free()
    return x, it, res, rc


def csr_of(P):
    return SimpleNamespace(n_rows=P.A.shape[0], n_cols=P.A.shape[1], rowptr=P.A.indptr.astype(np.int64), col=P.A.indices.astype(np.int32),
                           val=P.A.data)


def residual_as_the_device_forms_it(P, x):
    """|b - A x|_2 with every row summed in stored (ascending column) order, products and sums rounded one by one, as the
    lattice product does; then b - t and the norm"""
    A = P.A
    n = A.shape[0]
    lens = np.diff(A.indptr)
    t = np.zeros(n)
    for k in range(int(lens.max())):
        rows = np.flatnonzero(lens > k)
        e = A.indptr[rows] + k
        t[rows] = t[rows] + A.data[e] * x[A.indices[e]]
    r = P.b - t
    return float(np.sqrt(np.sum(r.astype(np.longdouble) ** 2)))


# ---- the passes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", F.SHAPES, ids=SHAPE_IDS)
def test_transform_every_axis(shape):
    P = F.problem(shape)
    c = direct_context(shape)
    n = len(P.b)
    src, dst = c.vector(n, P.b), c.vector(n)
    worst = 0.0
    for axis in range(3):
        dst.upload(np.full(n, np.nan))
        c.coarse_direct_transform(axis, dst, src)
        y = dst.download()
        y_ref, bound = F.transform_reference(shape, P.b, axis)
        assert np.isnan(y[P.boundary]).all(), (axis, "boundary rows of dst were written")
        err = np.abs(y[P.interior].astype(np.longdouble) - y_ref[P.interior])
        assert not np.isnan(y[P.interior]).any(), axis
        ratio = float((err / bound[P.interior]).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (axis, ratio, int(np.argmax(err / bound[P.interior])))
    print(f"{F.shape_id(shape)}: worst |y - y_ref| / bound over the three axes {worst:.3g}")
    src.free(); dst.free()
    c.close()


@pytest.mark.parametrize("shape", LANE_SHAPES, ids=[F.shape_id(s) for s in LANE_SHAPES])
def test_lane_map_with_unit_vectors(shape):
    """a unit vector at an interior vertex with three distinct coordinates: exactly zero off the line through it along the
    transformed axis, the bits of the table's column on it (products with 1.0 and 0.0 are exact)"""
    nx, ny, nz = shape
    at = [{4: 3, 17: 14, 33: 21}[v - 2] for v in shape]  # interior index (1-based) per axis, the largest beyond the first tile
    c = direct_context(shape)
    n = nx * ny * nz
    e = np.zeros((nz, ny, nx))
    e[at[2], at[1], at[0]] = 1.0
    src, dst = c.vector(n, e.ravel()), c.vector(n)
    for axis in range(3):
        S = capi().coarse_direct_tables(shape[axis] - 1)[0]
        want = np.zeros((nz, ny, nx))
        line = [at[2], at[1], at[0]]
        line[2 - axis] = slice(1, shape[axis] - 1)
        want[tuple(line)] = S[:, at[axis] - 1]
        dst.upload(np.full(n, np.nan))
        c.coarse_direct_transform(axis, dst, src)
        y = dst.download().reshape(nz, ny, nx)
        inner = y[1:-1, 1:-1, 1:-1]
        assert np.array_equal(inner, want[1:-1, 1:-1, 1:-1]), (axis, int(np.sum(inner != want[1:-1, 1:-1, 1:-1])))
    src.free(); dst.free()
    c.close()


# ---- the solve ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", F.SHAPES, ids=SHAPE_IDS)
def test_solve_meets_both_bounds(shape):
    C = capi()
    P = F.problem(shape)
    c = direct_context(shape)
    c.stats_reset()
    x, it, res, rc = solve(c, P.b)
    assert rc == C.OK and it == 0
    st = c.stats()
    assert int(st.coarse_solver) == 1 and int(st.coarse_solves) == 1 and int(st.coarse_iterations) == 0
    r2, e2 = F.solve_errors(P, x)
    print(f"{F.shape_id(shape)}: residual {r2:.3e} = {r2 / P.tol_res:.3g} bounds, error {e2:.3e} = {e2 / P.tol_x:.3g} bounds")
    assert r2 <= P.tol_res and e2 <= P.tol_x, (r2 / P.tol_res, e2 / P.tol_x)
    assert np.array_equal(x[P.boundary], (P.b / P.diag)[P.boundary])
    want = residual_as_the_device_forms_it(P, x)
    assert abs(res - want) <= 1e-9 * want, (res, want)
    # without the residual: the same bits, nothing else reported
    x2, it2, res2, rc2 = solve(c, P.b, want_residual=False)
    assert rc2 == C.OK and it2 == 0 and res2 == 0.0 and np.array_equal(x, x2)
    # b = 0: +0.0 everywhere, over the canaries
    x0, it0, res0, rc0 = solve(c, np.zeros(len(P.b)))
    assert rc0 == C.OK and it0 == 0 and res0 == 0.0
    assert np.array_equal(x0, np.zeros(len(P.b))) and not np.signbit(x0).any()
    c.close()


@pytest.mark.parametrize("shape", [(19, 6, 35), (7, 121, 7)], ids=["19x6x35", "7x121x7"])
def test_same_bits_run_to_run_and_for_any_grid(shape):
    P = F.problem(shape)
    c = direct_context(shape)
    first = solve(c, P.b)[0]
    assert np.array_equal(first, solve(c, P.b)[0])
    for cap in (1, 3, 0):
        c.set_option("coarse_direct_max_blocks", cap)
        assert np.array_equal(first, solve(c, P.b)[0]), cap
    c.close()
    c = direct_context(shape)  # a context of its own
    assert np.array_equal(first, solve(c, P.b)[0])
    c.close()


# ---- selection and refusals -------------------------------------------------------------------------------------------------

def refused(c, why):
    C = capi()
    with pytest.raises(C.GMGError) as e:
        c.set_coarse_solver(C.COARSE_DIRECT)
    assert e.value.code == C.ERR_UNSUPPORTED, e.value
    assert why in str(e.value), e.value


def cg_runs(c, b, iterations=None):
    """the coarse CG is what runs: (iterations > 0, stats say CG); returns the count"""
    x, it, res, rc = solve(c, b)
    assert rc == capi().OK and it > 0 and int(c.stats().coarse_solver) == 0 and res <= 1e-10
    if iterations is not None:
        assert it == iterations
    return it


def test_refusals_leave_the_cg_running():
    C = capi()
    shape = (7, 34, 5)
    P = F.problem(shape)
    # a level 0 uploaded as CSR
    c = C.Context(1)
    c.set_level_matrix(0, csr_of(P))
    its = cg_runs(c, P.b)
    refused(c, "gmg_set_level_matrix_lattice")
    cg_runs(c, P.b, its)
    c.close()
    # a Ke that is not separable (symmetric still)
    Ke = F.cell_matrix().copy()
    Ke[0, 7] *= 1.0 + 1e-6  # (the coupling of two opposite corners; the edge couplings of this matrix are zero)
    Ke[7, 0] = Ke[0, 7]
    c = C.Context(1)
    c.set_level_matrix_lattice(0, shape, Ke)
    its = cg_runs(c, P.b)
    refused(c, "separable")
    cg_runs(c, P.b, its)
    c.close()
    # more than 1024 vertices in a direction (fewer than 5 never form a lattice level 0: gmg_set_level_matrix_lattice refuses them)
    with pytest.raises(C.GMGError) as e:
        C.Context(1).set_level_matrix_lattice(0, (4, 5, 5), F.cell_matrix())
    assert e.value.code == C.ERR_INVALID
    big = (1025, 5, 5)
    bb = F.rhs(big)
    c = C.Context(1)
    c.set_level_matrix_lattice(0, big, F.cell_matrix())
    its = cg_runs(c, bb)
    refused(c, "1024")
    cg_runs(c, bb, its)
    c.close()
    # a communicator whose level 0 is partitioned
    c = C.Context(1)
    c.comm_init(0, 1, C.Context.unique_id())
    c.set_global_sizes(len(P.b), len(P.b))
    c.set_level_matrix(0, csr_of(P))
    its = cg_runs(c, P.b)
    refused(c, "partitioned")
    cg_runs(c, P.b, its)
    c.close()
    # selected first, partitioned afterwards: the selection is dropped
    c = direct_context(shape)
    assert solve(c, P.b)[1] == 0
    c.comm_init(0, 1, C.Context.unique_id())
    c.set_global_sizes(len(P.b), len(P.b))
    cg_runs(c, P.b, its)
    c.close()


def test_invalid_arguments():
    C = capi()
    L = C.load()
    import ctypes

    assert L.gmg_set_coarse_solver(None, 1) == C.ERR_INVALID
    assert L.gmg_coarse_direct_tables(ctypes.c_int(10), None, None, None) == C.ERR_INVALID
    assert L.gmg_coarse_direct_separable(None, None) == C.ERR_INVALID
    c = C.Context(1)
    with pytest.raises(C.GMGError) as e:  # before any level 0
        c.set_coarse_solver(C.COARSE_DIRECT)
    assert e.value.code == C.ERR_INVALID
    c.set_level_matrix_lattice(0, (7, 34, 5), F.cell_matrix())
    with pytest.raises(C.GMGError) as e:
        c.set_coarse_solver(2)
    assert e.value.code == C.ERR_INVALID
    v = c.vector(7 * 34 * 5, np.zeros(7 * 34 * 5))
    w = c.vector(7 * 34 * 5, np.zeros(7 * 34 * 5))
    with pytest.raises(C.GMGError) as e:  # not selected yet
        c.coarse_direct_transform(0, w, v)
    assert e.value.code == C.ERR_INVALID
    c.set_coarse_solver(C.COARSE_DIRECT)
    assert L.gmg_coarse_direct_transform(c.h, 0, None, v.ptr) == C.ERR_INVALID
    assert L.gmg_coarse_direct_transform(c.h, 0, v.ptr, None) == C.ERR_INVALID
    assert L.gmg_coarse_direct_transform(None, 0, w.ptr, v.ptr) == C.ERR_INVALID
    for bad_axis in (-1, 3):
        with pytest.raises(C.GMGError) as e:
            c.coarse_direct_transform(bad_axis, w, v)
        assert e.value.code == C.ERR_INVALID
    with pytest.raises(C.GMGError) as e:
        c.coarse_direct_transform(0, v, v)
    assert e.value.code == C.ERR_INVALID
    v.free(); w.free()
    c.close()


def test_reset_new_matrix_and_option_key():
    C = capi()
    shape = (7, 34, 5)
    P = F.problem(shape)
    c = direct_context(shape)
    assert solve(c, P.b)[1] == 0
    # back to the CG by hand
    c.set_coarse_solver(C.COARSE_CG)
    its = cg_runs(c, P.b)
    c.set_coarse_solver(C.COARSE_DIRECT)
    assert solve(c, P.b)[1] == 0
    # gmg_reset returns the context to the CG
    c._chk(c.L.gmg_reset(c.h, 1))
    c.set_level_matrix_lattice(0, shape, F.cell_matrix())
    cg_runs(c, P.b, its)
    # so does a new level-0 matrix
    c.set_coarse_solver(C.COARSE_DIRECT)
    c.set_level_matrix_lattice(0, shape, F.cell_matrix())
    cg_runs(c, P.b, its)
    c.set_coarse_solver(C.COARSE_DIRECT)
    c.set_level_matrix(0, csr_of(P))
    cg_runs(c, P.b)
    # the option key: the direct solver where the next lattice level 0 qualifies, silently the CG where it does not
    c.set_option("coarse_direct", 1)
    c.set_level_matrix_lattice(0, shape, F.cell_matrix())
    x, it, res, rc = solve(c, P.b)
    assert rc == C.OK and it == 0 and int(c.stats().coarse_solver) == 1
    Ke = F.cell_matrix().copy()
    Ke[0, 7] *= 1.0 + 1e-6  # (the coupling of two opposite corners; the edge couplings of this matrix are zero)
    Ke[7, 0] = Ke[0, 7]
    c.set_level_matrix_lattice(0, shape, Ke)
    cg_runs(c, P.b)
    c.set_level_matrix(0, csr_of(P))
    cg_runs(c, P.b)
    c.set_option("coarse_direct", 0)
    c.set_level_matrix_lattice(0, shape, F.cell_matrix())
    cg_runs(c, P.b, its)
    c.close()


# ---- whole runs ---------------------------------------------------------------------------------------------------------------

def adaptive_run(coarse_solver):
    """8 atoms, 45^3 level 0, two adaptive cycles: per cycle (outer iterations, coarse iterations, coarse solver, true
    residual / ||b||)"""
    S = pkg().step50
    kw = dict(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=2, r_c=0.5,
              cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR")
    if coarse_solver is not None:
        kw["coarse_solver"] = coarse_solver
    p = S.Problem(S.prm_text(**kw))
    out = []
    try:
        p.set_nacl_atoms(1)
        import scipy.sparse as sp

        for cycle in range(2):
            rep = p.run_cycle(cycle, on_device=True)
            m, b, u = p.matrix("system"), p.vector("rhs"), p.vector("solution")
            A = sp.csr_matrix((m.val, m.col, m.rowptr), shape=(m.n_rows, m.n_cols))
            free = ~p.constrained_mask()
            # (the solution is read after constraints.distribute: the rows of constrained DoFs are diagonal with rhs 0 and
            # their columns are eliminated, so the residual is that of the unconstrained rows)
            r = (b - A @ u)[free]
            out.append((rep["cg_iterations"], rep["coarse_iterations"], rep["coarse_solver"], float(np.linalg.norm(r) / np.linalg.norm(b))))
        log = p.log()
    finally:
        p.close()
    return out, log


def test_whole_runs_with_and_without_the_key():
    base, _ = adaptive_run(None)
    direct, log = adaptive_run("direct")
    print("default (outer, coarse its, solver, |b - A u| / |b|) per cycle:", base)
    print("direct  (outer, coarse its, solver, |b - A u| / |b|) per cycle:", direct)
    assert "not applicable" not in log
    for cycle in range(2):
        assert base[cycle][2] == 0 and base[cycle][1] > 0
        assert direct[cycle][2] == 1 and direct[cycle][1] == 0
        assert abs(base[cycle][0] - direct[cycle][0]) <= 1, (cycle, base[cycle][0], direct[cycle][0])
        assert base[cycle][3] <= 1.001e-8 and direct[cycle][3] <= 1.001e-8, (cycle, base[cycle][3], direct[cycle][3])


def test_key_says_once_where_it_does_not_apply():
    """level 0 assembled on the host and uploaded as CSR: both cycles go on with the coarse CG, and the log says so once"""
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=2,
                             r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="Jacobi",
                             level0_on_device=False, coarse_solver="direct"))
    try:
        p.set_nacl_atoms(1)
        for cycle in range(2):
            rep = p.run_cycle(cycle, on_device=True)
            assert rep["coarse_solver"] == 0 and rep["coarse_iterations"] > 0
        assert p.log().count("Coarse solver direct: not applicable (") == 1 and "), coarse CG" in p.log()
    finally:
        p.close()


# ---- life cycle -----------------------------------------------------------------------------------------------------------------

def test_no_leak_across_select_solve_reset_rounds():
    import torch

    C = capi()
    shape = (19, 6, 35)
    P = F.problem(shape)

    def one_round():
        c = C.Context(1)
        try:
            c.set_level_matrix_lattice(0, shape, F.cell_matrix())
            c.set_coarse_solver(C.COARSE_DIRECT)
            assert solve(c, P.b)[1] == 0
            c.set_coarse_solver(C.COARSE_CG)
            c.set_coarse_solver(C.COARSE_DIRECT)
            c._chk(c.L.gmg_reset(c.h, 1))
            c.set_option("coarse_direct", 1)
            c.set_level_matrix_lattice(0, (7, 34, 5), F.cell_matrix())
            assert solve(c, F.problem((7, 34, 5)).b)[1] == 0
        finally:
            c.close()

    free = []
    for _ in range(6):
        one_round()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    print("free device memory after each round, relative to the first:", [f - free[0] for f in free])
    assert free[-1] == free[0], free
