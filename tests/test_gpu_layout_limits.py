"""The device layouts behind gmg_spmv on operators that sit exactly on the limits of their planner (csrc/gmg_layout.hpp), one on
either side of each limit: the last dictionary code, a 16-bit column offset of 65535, the last class of the LDS tables of
the pattern-run and the lattice kernel, the 64th slice of a wave, slices without quads, rows that end at the edge of the LDS row
window, 1024 rows and the 12 % padding bound (tests/layout_limit_cases.py).  Every case asserts the layout it
got -- a case that drifts off its limit fails --, compares the product bit for bit with the oracle's CSR product and with the
device's own CSR kernel; the square operators also go through the smoother epilogues and the coarse CG.  Options sell_grid and
sellp_cost reach the planner from here."""
import functools
import re

import numpy as np
import pytest

import layout_limit_cases as L
from gpu_util import capi
from oracle import gmg_oracle as go

pytestmark = pytest.mark.gpu

SQUARE = [name for name, c in L.CASES.items() if c.square]


def context(n_levels, options, debug=False):
    c = capi().Context(n_levels)
    for key, value in options:
        c.set_option(key, value)
    if debug:
        c.set_option("debug_upload", 1)
    return c


def logged(capfd, fn):
    """what fn() writes to standard error: the debug_upload lines"""
    capfd.readouterr()
    fn()
    return capfd.readouterr().err


def operator_lines(err, m):
    """the flags of the "[gmg] operator" lines of uploads of m, one dict per upload"""
    pat = r"\[gmg\] operator %d x %d nnz %d: tiles (\d+) grid \d+ sell (\d) val8 (\d) col16 (\d) sell_grid (\d+) patterns \d+ pattern_slices (\d+)/(\d+)" % (
        m.n_rows, m.n_cols, m.nnz)
    return [dict(tiles=int(t), layout=(L.SELL * int(s) + L.VAL8 * int(v) + L.COL16 * int(c)) if int(s) else 0, sell_grid=int(g),
                 pattern_slices=int(ps), slices=int(ns))
            for t, s, v, c, g, ps, ns in re.findall(pat, err)]


def check_class_lines(case, err, count=1):
    """the class counts the planner printed: those of the case, `count` times (None: the line must not appear)"""
    sellp = [int(k) for k in re.findall(r"row classes of the run-pattern slices: (\d+)", err)]
    lattice = [int(k) for k in re.findall(r"lattice interior: .* (\d+) classes,", err)]
    refused = [int(k) for k in re.findall(r"lattice interior not used: .* classes (-?\d+)", err)]
    assert sellp == ([case.sellp_classes] * count if case.sellp_classes is not None else []), sellp
    assert lattice == ([case.lattice_classes] * count if case.lattice_classes is not None else []), lattice
    if case.lattice_refused is not None:
        assert refused == [case.lattice_refused] * count, refused


def vector_for(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


@functools.lru_cache(maxsize=None)
def product_reference(op):
    m = L.operator(op)
    x = vector_for(m.n_cols, 101)
    x.setflags(write=False)
    y = go.spmv(m, x)
    y.setflags(write=False)
    return x, y


def empty_rows(m):
    return np.diff(m.rowptr) == 0


@pytest.mark.parametrize("name", list(L.CASES))
def test_product_at_the_limit(name, capfd):
    """y = A x on level 0: the layout bits and class counts of the case, every row written, the oracle's bits; rows that store
    nothing come out +0.0; the device's CSR row-window kernel (disable_sell) gives the same bits."""
    case = L.CASES[name]
    m = L.operator(case.op)
    x, ref = product_reference(case.op)
    c = context(1, case.options, debug=True)
    err = logged(capfd, lambda: c.set_level_matrix(0, m))
    lay = int(c.stats().spmv0_layout)
    assert lay == case.layout, (name, lay, case.layout)
    check_class_lines(case, err)
    lines = operator_lines(err, m)
    assert len(lines) == 1 and lines[0]["layout"] == case.layout & 7
    # the slices with a column pattern; 0 of them: every column comes from the stream
    assert (lines[0]["pattern_slices"], lines[0]["slices"]) == (case.pattern_slices, (m.n_rows + 63) // 64 if case.layout else 0), lines
    if dict(case.options).get("sell_grid") and case.layout:
        assert lines[0]["sell_grid"] == 8
    vx, vy = c.vector(m.n_cols, x), c.vector(m.n_rows, np.full(m.n_rows, np.nan))
    c.spmv(0, vy, vx)
    y = vy.download()
    c.close()
    assert not np.isnan(y).any(), f"{int(np.isnan(y).sum())} rows were not written, first {int(np.argmax(np.isnan(y)))}"
    bad = np.nonzero(y != ref)[0]
    assert bad.size == 0, (name, bad[:10], y[bad[:3]], ref[bad[:3]])
    assert not y[empty_rows(m)].view(np.uint64).any()  # +0.0, not -0.0
    c2 = context(1, (("disable_sell", 1),))
    c2.set_level_matrix(0, m)
    assert int(c2.stats().spmv0_layout) == 0
    vx2, vy2 = c2.vector(m.n_cols, x), c2.vector(m.n_rows, np.full(m.n_rows, np.nan))
    c2.spmv(0, vy2, vx2)
    y2 = vy2.download()
    c2.close()
    assert np.array_equal(y2, y)


@functools.lru_cache(maxsize=None)
def smoother_reference(op, kind, steps, degree, from_zero):
    m = L.operator(op)
    mg = go.OracleMG(L.two_level_hierarchy(m), smoother=kind, omega=0.5, steps=steps, cheb_degree=degree)
    u0, rhs = vector_for(m.n_rows, 102), vector_for(m.n_rows, 103)
    ref = mg.smooth(1, u0, rhs, from_zero)
    for a in (u0, rhs, ref):
        a.setflags(write=False)
    return u0, rhs, ref


@pytest.mark.parametrize("name", SQUARE)
def test_smoother_epilogues_at_the_limit(name, capfd):
    """One damped-Jacobi and one Chebyshev step (epilogues of the SpMV kernels) with the operator as level 1 of a two-level
    hierarchy, two steps (Chebyshev: degree 3), from zero and not from zero, bit for bit against the oracle's smoother.

    The operators with empty slices have rows without a diagonal: the inverse diagonal is infinite there on both sides, and
    whatever a smoother returns is infinite in those rows.  The layouts pad with explicit +0.0 entries, which is exact for
    finite x only (gmg_layout.hpp): a product over such an iterate turns 0 * inf into NaN in the 78 rows beside the empty
    slices where a CSR sum stays finite.  That is the layouts' precondition, so these operators take the steps whose products
    read a finite x: one Jacobi step that does not start from zero (the Jacobi epilogue over u), and one Chebyshev step of
    degree 1 that does not start from zero (the residual epilogue r = rhs - A u over u, then r / diagonal / theta).  What
    cannot run is a second chained step and the Chebyshev product of degree >= 2, whose input is r / diagonal.  The empty rows
    come out infinite on both sides (infinities compare equal, a NaN on either side fails), every other row must carry the
    oracle's bits."""
    case = L.CASES[name]
    m = L.operator(case.op)
    hier = L.two_level_hierarchy(m)
    c = context(2, case.options, debug=True)
    err = logged(capfd, lambda: c.load_hierarchy(hier))
    c.set_option("debug_upload", 0)
    lines = operator_lines(err, m)  # the system matrix, then level 1
    assert len(lines) == 2 and lines[1]["layout"] == case.layout & 7 and lines[1]["pattern_slices"] == case.pattern_slices, lines
    check_class_lines(case, err, count=2 if lines[0]["layout"] else 1)
    # (kind, steps, Chebyshev degree, from zero); kind 0: Jacobi, 2: Chebyshev
    runs = [(0, 1, 3, False), (2, 1, 1, False)] if empty_rows(m).any() else [(kind, 2, 3, from_zero) for kind in (0, 2) for from_zero in (True, False)]
    for kind, steps, degree, from_zero in runs:
        c.set_smoother(kind, 0.5, steps, cheb_degree=degree)
        u0, rhs, ref = smoother_reference(case.op, kind, steps, degree, from_zero)
        u, r = c.vector(m.n_rows, u0), c.vector(m.n_rows, rhs)
        c.smoother_step(1, u, r, from_zero)
        got = u.download()
        assert not np.isnan(got).any() and np.isinf(got[empty_rows(m)]).all() and np.isfinite(got[~empty_rows(m)]).all()
        bad = np.nonzero(got != ref)[0]
        assert bad.size == 0, (name, kind, from_zero, bad[:10], got[bad[:3]], ref[bad[:3]])
    c.close()


@functools.lru_cache(maxsize=None)
def coarse_reference(op):
    m = L.operator(op)
    b = vector_for(m.n_rows, 104)
    b[empty_rows(m)] = 0.0  # a row that stores nothing has no equation: the system is solvable only with a zero there
    x, it, res, rc = go.OracleMG(L.one_level_hierarchy(m)).coarse_solve(b)
    assert rc == 0 and it > 5
    b.setflags(write=False)
    x.setflags(write=False)
    return b, x, it


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("name", SQUARE)
def test_coarse_cg_at_the_limit(name, variant):
    """The coarse CG with the operator as level 0, in each of its kernel arrangements: the oracle's iteration count and its
    solution to the 1e-9 relative bound of tests/test_gpu_lattice.py."""
    case = L.CASES[name]
    m = L.operator(case.op)
    b, x_ref, it_ref = coarse_reference(case.op)
    c = context(1, case.options)
    c.set_tuning(cg_variant=variant)
    c.set_level_matrix(0, m)
    assert int(c.stats().spmv0_layout) == case.layout
    vb, vx = c.vector(m.n_rows, b), c.vector(m.n_rows)
    it, res, rc = c.coarse_solve(vx, vb)
    x = vx.download()
    c.close()
    assert rc == 0 and it == it_ref, (name, variant, rc, it, it_ref)
    assert np.abs(x - x_ref).max() <= 1e-9 * np.abs(x_ref).max()


def check_window_product(m, y, ref, x_max):
    """rows that fit the window: bit for bit; a row beyond it goes through the strided path: the bound of
    test_csr_window_irregular_empty_and_long_rows"""
    assert not np.isnan(y).any()
    fits = np.array([L.fits_window(m.rowptr, r) for r in range(m.n_rows)])
    assert (~fits).sum() >= 8
    bad = np.nonzero(fits & (y != ref))[0]
    assert bad.size == 0, (bad[:10], y[bad[:3]], ref[bad[:3]])
    cs = np.concatenate(([0.0], np.cumsum(np.abs(m.val))))
    abs_row = (cs[m.rowptr[1:]] - cs[m.rowptr[:-1]])[~fits]  # sum |val| of the long row itself
    assert (np.abs(y - ref)[~fits] <= 1e-12 * abs_row * x_max).all()


@pytest.mark.parametrize("last_align", [0, 1, 2, 3])
@pytest.mark.parametrize("length", L.WINDOW_LENGTHS)
def test_row_window_at_its_edge(length, last_align, capfd):
    """Rows of 4092 .. 4097 entries that start at every offset from a multiple of four, as the first, a middle and the last row,
    followed or not by short rows of the same tile, and runs of 1023, 1024 and 1025 empty rows, on the CSR row-window kernel:
    through spmv, through prolongate, and through restrict_and_add (the transposed operator as the prolongation), where the
    sum starts from the destination's value."""
    m = L.window_operator(length, length, last_align)
    assert m.rowptr[-2] % 4 == last_align and m.rowptr[1] == length
    tiles = L.window_tiles(m.rowptr)
    x = vector_for(m.n_cols, 105)
    ref = go.spmv(m, x)
    c = context(2, (), debug=True)
    err = logged(capfd, lambda: c.set_level_matrix(0, m))
    c.set_option("debug_upload", 0)
    assert int(c.stats().spmv0_layout) == 0
    assert [ln["tiles"] for ln in operator_lines(err, m)] == [len(tiles) - 1]
    vx, vy = c.vector(m.n_cols, x), c.vector(m.n_rows, np.full(m.n_rows, np.nan))
    c.spmv(0, vy, vx)
    check_window_product(m, vy.download(), ref, np.abs(x).max())
    # prolongation = the operator itself: fine level = its rows, coarse level = its columns
    c.set_level_matrix(0, L.tridiagonal(m.n_cols))
    c.set_level_matrix(1, L.tridiagonal(m.n_rows))
    c.set_prolongation(0, m)
    vy.upload(np.full(m.n_rows, np.nan))
    c.prolongate(0, vy, vx)
    check_window_product(m, vy.download(), ref, np.abs(x).max())
    c.close()
    # prolongation = the transposed operator: restrict_and_add applies the operator itself, starting from the destination
    mt = L.transpose(m)
    c0 = vector_for(m.n_rows, 106)
    ref_add = go.spmv_transpose(mt, x, c0)
    c = context(2, ())
    c.set_level_matrix(0, L.tridiagonal(m.n_rows))
    c.set_level_matrix(1, L.tridiagonal(m.n_cols))
    c.set_prolongation(0, mt)
    vf, vc = c.vector(m.n_cols, x), c.vector(m.n_rows, c0)
    c.restrict_and_add(0, vc, vf)
    check_window_product(m, vc.download(), ref_add, np.abs(x).max())
    c.close()
