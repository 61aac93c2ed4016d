"""tests/fastdiag_reference.py is a yardstick the GPU tests of the direct coarse solver stand on: here, without a GPU, the
numpy restatement of the definition is shown to meet both solve bounds on every shape and to miss them by more than 100 x
when an eigenvalue is wrong by 1e-6 or two axes are confused; the host-side tables of the library
(gmg_coarse_direct_tables) are held against mpmath, and the separability check against the host's own cell matrix."""
import numpy as np
import pytest

import fastdiag_reference as F
from gpu_util import capi, pkg

SHAPE_IDS = [F.shape_id(s) for s in F.SHAPES]


def ulp_distance(a, ref):
    """|a - ref| in units of the spacing of doubles at ref (ref in higher precision)"""
    ref64 = np.asarray(ref, dtype=np.float64)
    return np.abs(np.asarray(a, dtype=np.longdouble) - ref) / np.spacing(np.abs(ref64)).astype(np.longdouble)


@pytest.mark.parametrize("shape", F.SHAPES, ids=SHAPE_IDS)
def test_restatement_meets_both_bounds(shape):
    P = F.problem(shape)
    x = F.fastdiag_solve(shape, P.b, P.diag)
    res, err = F.solve_errors(P, x)
    ref_res, _ = F.solve_errors(P, P.x_ref)
    print(f"{F.shape_id(shape)}: kappa {P.kappa:.4g}  residual {res:.3e} (bound {P.tol_res:.3e}, reference's own {ref_res:.3e})  "
          f"error {err:.3e} (bound {P.tol_x:.3e})")
    assert ref_res <= 0.01 * P.tol_res  # the reference stays well inside its own bound
    assert res <= P.tol_res and err <= P.tol_x
    assert np.array_equal(x[P.boundary], (P.b / P.diag)[P.boundary])


@pytest.mark.parametrize("shape", F.SHAPES, ids=SHAPE_IDS)
def test_one_wrong_eigenvalue_breaks_the_bounds(shape):
    """one lambda off by 1e-6 relative -- the middle one of the longest axis, where lambda is of the size of D; the lowest
    ones of a long axis next to two short ones barely show in D -- : both bounds are missed by more than 100 x"""
    P = F.problem(shape)
    axis = int(np.argmax(P.m))
    tabs = [list(F.tables_float64(v - 1)) for v in shape]
    tabs[axis][1] = tabs[axis][1].copy()
    tabs[axis][1][P.m[axis] // 2] *= 1.0 + 1e-6
    res, err = F.solve_errors(P, F.fastdiag_solve(shape, P.b, P.diag, tabs))
    print(f"{F.shape_id(shape)}: residual {res / P.tol_res:.3g} bounds, error {err / P.tol_x:.3g} bounds")
    assert res >= 100 * P.tol_res and err >= 100 * P.tol_x, (res / P.tol_res, err / P.tol_x)


def test_confused_axes_break_the_bounds():
    """(19, 6, 35): the tables of x and z swapped.  Their sizes differ (m = 17 and 33), so the swap can only be applied with
    the vector read as a (35, 6, 19) lattice -- the mistake of a kernel that confuses the strides of two axes."""
    shape = (19, 6, 35)
    P = F.problem(shape)
    x = F.fastdiag_solve(shape[::-1], P.b, P.diag)
    res, err = F.solve_errors(P, x)
    assert res >= 100 * P.tol_res and err >= 100 * P.tol_x, (res / P.tol_res, err / P.tol_x)


@pytest.mark.parametrize("n", [4, 17, 18, 34, 120, 1023])
def test_tables_against_high_precision(n):
    """entries within 4 ulp of mpmath (longdouble where mpmath is not importable); S^T S = I within (m + 4) u"""
    m = n - 1
    S, lam, mu = capi().coarse_direct_tables(n)
    try:
        import mpmath as mp

        mp.mp.dps = 40
        ks = range(1, n)
        # S[j][k] depends on (j k) mod 2n only: 2n values
        by_r = np.array([np.longdouble(mp.nstr(mp.sqrt(mp.mpf(2) / n) * mp.sin(mp.pi * r / n), 30)) for r in range(2 * n)])
        by_r[[0, n]] = 0  # sin(0) and sin(pi): exactly zero, which mpmath's rounded pi does not return
        S_ref = by_r[np.outer(np.arange(1, n), np.arange(1, n)) % (2 * n)]
        lam_ref = np.array([np.longdouble(mp.nstr(2 - 2 * mp.cos(mp.pi * k / n), 30)) for k in ks])
        mu_ref = np.array([np.longdouble(mp.nstr((4 + 2 * mp.cos(mp.pi * k / n)) / 6, 30)) for k in ks])
    except ImportError:
        S_ref, lam_ref, mu_ref = F.tables_longdouble(n)
    for got, ref, what in ((S, S_ref, "S"), (lam, lam_ref, "lambda"), (mu, mu_ref, "mu")):
        d = ulp_distance(got, ref)
        assert d.max() <= 4, (what, float(d.max()))
    assert np.array_equal(S, S.T)
    if m <= 200:
        Sl = S.astype(np.longdouble)
        assert np.abs(Sl.T @ Sl - np.eye(m)).max() <= (m + 4) * F.U
    else:  # (longdouble products of this size are slow: columns sampled)
        Sl = S.astype(np.longdouble)
        cols = [0, 1, m // 3, m - 2, m - 1]
        G = Sl.T @ Sl[:, cols]
        assert np.abs(G - np.eye(m)[:, cols]).max() <= (m + 4) * F.U


def test_tables_refuse_bad_sizes():
    C = capi()
    for n in (3, 1024, 0, -5):
        with pytest.raises(C.GMGError) as e:
            C.coarse_direct_tables(n)
        assert e.value.code == C.ERR_INVALID


def host_level0_cell_matrix():
    """LaplaceProblem::level0_cell_matrix of BASELINE config 1 (45^3 level 0), through the arrays the driver hands to
    gmg_assemble_system_matrix: K_of_level[0] is that matrix"""
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=1,
                             r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="Jacobi"))
    try:
        p.set_nacl_atoms(1)
        p.run_cycle(0, on_device=False)
        return np.array(p.system_assembly_inputs().K_of_level[0])
    finally:
        p.close()


def test_separability_check():
    C = capi()
    Ke = host_level0_cell_matrix()
    s = C.coarse_direct_separable(Ke)
    assert s is not None and abs(s - 3.0 * Ke[0, 0]) == 0.0
    assert C.coarse_direct_separable(F.cell_matrix()) is not None
    assert C.coarse_direct_separable(7.5 * F.cell_matrix()) is not None
    for i, j in ((0, 0), (0, 7), (3, 5), (7, 7)):
        bad = Ke.copy()
        bad[i, j] *= 1.0 + 1e-10
        assert C.coarse_direct_separable(bad) is None, (i, j)
    assert C.coarse_direct_separable(-Ke) is None
    assert C.coarse_direct_separable(np.zeros((8, 8))) is None
    nan = Ke.copy()
    nan[2, 2] = np.nan
    assert C.coarse_direct_separable(nan) is None
