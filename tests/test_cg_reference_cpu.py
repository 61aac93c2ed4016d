"""tests/cg_reference.py against itself and against the oracle: the tiers agree, the fp64 tier reproduces the oracle's coarse
solve on the 45^3 lattice, and every case of tests/test_gpu_coarse_cg.py is targetable (stops at its iteration in every tier
with the margin of target_tol) and sensitive (no single step alpha_j d_j is smaller than 100 tolerances on x)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import cg_reference as R
import rank_cases as RC
from oracle import gmg_oracle as go
from oracle import step50_oracle as so


def test_target_tol_is_the_geometric_mean_and_refuses_a_narrow_margin():
    h = [4.0, 2.0, 3.0, 1.0, 0.99, 1e-3]
    assert R.target_tol(h, 1) == pytest.approx(np.sqrt(2.0 * 4.0))
    assert R.target_tol(h, 3) == pytest.approx(np.sqrt(1.0 * 2.0))
    assert R.target_tol(h, 5) == pytest.approx(np.sqrt(1e-3 * 0.99))
    for k in (2, 4):  # a residual that went up, one that fell by 1 % only
        with pytest.raises(ValueError):
            R.target_tol(h, k)
    for k in (0, 6):
        with pytest.raises(ValueError):
            R.target_tol(h, k)


def test_small_dense_solve():
    """n steps solve an n x n system; the result is that of numpy.linalg.solve"""
    m, _ = R.operator("tri3")
    A = np.zeros((3, 3))
    A[np.repeat(np.arange(3), np.diff(m.rowptr)), m.col] = m.val
    b = R.rhs("tri3")
    for tier in R.TIERS:
        for pc in R.PRECONDS.values():
            r = R.cg(m, b, 1e-14, 10, precond=pc, tier=tier)
            assert r.status == R.OK and r.iterations == 3 and len(r.history) == 4 and len(r.steps) == 3
            assert np.abs(r.x - np.linalg.solve(A, b)).max() <= 1e-15
            assert np.array_equal(r.x, (r.steps[0] + r.steps[1]) + r.steps[2]) or tier == "ld"
    x0 = np.linalg.solve(A, b)
    r = R.cg(m, b, 1e-14, 10, x0=x0)
    assert (r.iterations, r.status) == (0, R.OK) and np.array_equal(r.x, x0)


def test_entry_and_failure_conditions():
    m, _ = R.operator("csr")
    b = R.rhs("csr")
    for tier in R.TIERS:
        r = R.cg(m, np.zeros(m.n_rows), 1e-10, 1000, tier=tier)
        assert (r.iterations, r.status, r.res) == (0, R.OK, 0.0) and not r.x.any()
        r = R.cg(m, b, 1e3, 1000, tier=tier)
        assert (r.iterations, r.status) == (0, R.OK) and not r.x.any() and abs(r.res - np.linalg.norm(b)) <= 1e-14 * r.res
        bn = b.copy(); bn[77] = np.nan
        r = R.cg(m, bn, 1e-10, 1000, tier=tier)
        assert (r.iterations, r.status) == (0, R.NOCONV) and np.isnan(r.res)
        r = R.cg(m, b, R.REFUSE_TOL, 5, tier=tier)
        assert (r.iterations, r.status) == (5, R.NOCONV) and len(r.steps) == 5
        # the iterate a refused solve leaves is the one a longer solve passes through
        longer = R.cg(m, b, R.REFUSE_TOL, 9, tier=tier)
        assert np.array_equal(longer.history[:6], r.history)


def test_fp64_tier_against_the_oracle_on_45_cubed(golden_dir):
    """MGCoarseGridIterativeSolver on BASELINE config 2's level 0: 97 iterations in both; the two are independent
    implementations of the same operation order in fp64, apart from the order inside the dot products"""
    q, p = so.read_lammps(os.path.join(golden_dir, "atom_n1_8.data"))
    hier = so.build_gaussian_cycle0(q, p, left=0, right=1, h=0.25, vacuum=10, r_c=0.5, cutoff_param=3.5, n_q_rhs=1, bc="Inhomogeneous")
    x_ref, it_ref, res_ref, rc_ref = go.OracleMG(hier).coarse_solve(hier.system_rhs)
    assert rc_ref == 0 and it_ref == 97
    for tier in ("seq", "pair"):
        r = R.cg(hier.level_matrices[0], hier.system_rhs, 1e-10, 1000, tier=tier, keep_steps=False)
        assert (r.iterations, r.status) == (97, R.OK)
        assert abs(r.res - res_ref) <= 1e-9 * res_ref
        assert np.abs(r.x - x_ref).max() <= 1e-12 * np.abs(x_ref).max()


def test_operators_are_symmetric_and_of_the_advertised_width():
    for name, width in (("sell", 27), ("band9", 9), ("tri513", 3), ("csr", 27), ("formed", 27)):
        m, _ = R.operator(name)
        n = m.n_rows
        length = np.diff(m.rowptr)
        assert length.max() == width and (np.median(length) == width or name in ("csr", "formed"))
        A = np.zeros((n, n))
        A[np.repeat(np.arange(n), length), m.col] = m.val
        assert np.array_equal(A, A.T)
        assert np.all(np.diff(m.col)[np.delete(np.arange(m.nnz - 1), m.rowptr[1:-1] - 1)] > 0)  # ascending inside a row
    # what keeps them on the paths the GPU cases are written for: SELL-64 is taken at 1024 rows and up to 12 % padding
    for name, sell in (("sell", True), ("band9", False), ("csr", False), ("lattice", True)):
        m, _ = R.operator(name)
        length = np.diff(m.rowptr)
        padded = sum((int(length[s:s + 64].max()) + 3) // 4 * 256 for s in range(0, m.n_rows, 64))
        assert m.n_rows >= 1024 and (padded <= 1.12 * m.nnz) == sell, (name, padded / m.nnz)


@pytest.mark.parametrize("case", R.gpu_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_every_gpu_case_is_targetable_and_sensitive(case):
    kind, name, k, pc, start = case
    tol_x = R.x_tolerance(name)
    ref = R.case_result(case)
    for tier in R.TIERS:
        r = R.case_result(case, tier)
        assert r.iterations == k and r.status == (R.OK if kind == "stop" else R.NOCONV), (tier, r.iterations, r.status)
        if kind == "stop":  # the margin holds in this tier's own history too
            tol = R.stop_case(name, k, pc, start)[0]
            assert r.history[k] <= tol / R.MARGIN and r.history[:k].min() >= R.MARGIN * tol
        assert np.abs(r.history - ref.history).max() <= 1e-9 * ref.history[0]
        assert np.abs(r.x - ref.x).max() <= tol_x / R.X_TOL_FACTOR * np.abs(ref.x).max()
    scale = np.abs(ref.x).max()
    smallest = min(np.abs(s).max() for s in ref.steps)
    assert smallest > R.SENSITIVITY * tol_x * scale, (smallest / (tol_x * scale))


@pytest.mark.parametrize("name,k", RC.coarse_pairs(), ids=lambda v: str(v))
def test_every_rank_case_is_targetable_and_sensitive(name, k):
    """the (operator, k) pairs tests/test_gpu_ranks_reference.py solves on a partitioned level 0 and gpu_cases() does not hold:
    the same proof, with the same tolerance on x and the same SENSITIVITY (the spread S stays that of gpu_cases())"""
    tol_x = RC.x_tolerance(name)
    tol, ref = RC.stop_case(name, k)
    for tier in R.TIERS:
        r = RC.stop_case(name, k, tier)[1]
        assert r.iterations == k and r.status == R.OK, (tier, r.iterations, r.status)
        assert r.history[k] <= tol / R.MARGIN and r.history[:k].min() >= R.MARGIN * tol
        assert np.abs(r.history - ref.history).max() <= 1e-9 * ref.history[0]
        assert np.abs(r.x - ref.x).max() <= tol_x / R.X_TOL_FACTOR * np.abs(ref.x).max()
    scale = np.abs(ref.x).max()
    smallest = min(np.abs(s).max() for s in ref.steps)
    assert smallest > R.SENSITIVITY * tol_x * scale, (smallest / (tol_x * scale))


@pytest.mark.parametrize("pc,what", [c for c in RC.LAYOUT_OUTER_CASES if c[1] != "b0"], ids=lambda v: str(v))
def test_every_layout_outer_case_is_targetable_and_sensitive(pc, what):
    """the outer CG cases tests/test_gpu_ranks_layouts.py solves on the partitioned hybrid operator: the same proof"""
    name = RC.LAYOUT_OUTER
    tol_x = RC.x_tolerance(name)
    tol, ref = RC.outer_case(name, pc, what)
    k = R.OUTER_MAX_IT if what == "max_it" else R.OUTER_K
    for tier in R.TIERS:
        r = RC.outer_case(name, pc, what, tier)[1]
        assert r.iterations == k and r.status == (R.NOCONV if what == "max_it" else R.OK), (tier, r.iterations, r.status)
        if what != "max_it":
            assert r.history[k] <= tol / R.MARGIN and r.history[:k].min() >= R.MARGIN * tol
        assert np.abs(r.history - ref.history).max() <= 1e-9 * ref.history[0]
        assert np.abs(r.x - ref.x).max() <= tol_x / R.X_TOL_FACTOR * np.abs(ref.x).max()
    scale = np.abs(ref.x).max()
    smallest = min(np.abs(s).max() for s in ref.steps)
    assert smallest > R.SENSITIVITY * tol_x * scale, (smallest / (tol_x * scale))


def test_layout_operators_are_symmetric_positive_definite():
    """the operators the layout groups solve on: the 21 x 17 x 40 lattice and the hybrid operator (strictly diagonally
    dominant with a positive diagonal, symmetric: SPD, so CG applies)"""
    for name in ("lat21", RC.LAYOUT_OUTER):
        m = RC.operator(name)
        n, length = m.n_rows, np.diff(m.rowptr)
        row = np.repeat(np.arange(n), length)
        key = np.sort(row * n + m.col)
        assert np.array_equal(key, np.sort(m.col.astype(np.int64) * n + row))            # the pattern is symmetric
        order, order_t = np.argsort(row * n + m.col), np.argsort(m.col.astype(np.int64) * n + row)
        assert np.array_equal(m.val[order], m.val[order_t])                               # and so are the values
        assert np.all(np.diff(m.col)[np.delete(np.arange(m.nnz - 1), m.rowptr[1:-1] - 1)] > 0)
        if name == RC.LAYOUT_OUTER:
            off = np.zeros(n)
            np.add.at(off, row[m.col != row], np.abs(m.val[m.col != row]))
            assert np.all(R.diagonal(m) > off) and length.max() == 84 and np.median(length) == 27


def test_spread_of_the_tiers_with_the_layout_cases():
    """S over the solves the layout groups add: it stays below the S of gpu_cases(), so the tolerance
    64 S on x is the same for them and nothing is widened"""
    S, S_new = R.spread(False), RC.layout_spread()
    print(f"layout cases: S = {S_new:.3e} against {S:.3e} of gpu_cases()")
    assert 0.0 < S_new <= S


def test_rank_sequence_cases_are_those_of_gpu_cases():
    """the sequence and the refused solve the ranks run on "csr" are cases of gpu_cases() already"""
    have = set(R.gpu_cases())
    for kind, k in R.SEQUENCE:
        assert kind == "zero" or (kind, "csr", k, "identity", "zero") in have


def test_converged_start_vector_case():
    for pc in R.PRECONDS:
        for tier in R.TIERS:
            x0, tol, r = R.converged_start_case(pc, tier)
            assert (r.iterations, r.status) == (0, R.OK) and np.array_equal(r.x, x0) and r.res <= tol / R.MARGIN


def test_spread_of_the_tiers():
    """S and the tolerance 64 S on x; the tiers differ by rounding only, so S is a small multiple of
    2^-53: a few hundred roundings at most over 25 iterations"""
    for large in (False, True):
        S = R.spread(large)
        print(f"{'200 000 rows' if large else 'all other cases'}: S = {S:.3e}, tolerance on x = {R.X_TOL_FACTOR * S:.3e} max|x|")
        assert 0.0 < S <= 512 * 2.0 ** -53
