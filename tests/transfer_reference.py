"""The Q1 level transfer P_l (level l -> l + 1) and its transpose, restated from the contract of gmg_build_transfer in
include/gmg_coulomb.h alone.  Nothing here calls the library under test, and nothing is taken from
csrc/gmg_transfer.hpp or from build_transfer in csrc/host/laplace_problem.cc.

Two evaluators that share no code (not even the CSR assembly or the key arithmetic):

    from_vertices   A, the definition: P[f, c] = prod_d max(0, 1 - |x_f,d - x_c,d| / H), H = 2 fine_spacing, 0 for a coarse
                    DoF flagged boundary; dense over all (fine, coarse) pairs in chunks.  Quadratic: small cases only.
    from_cells      B, the embedding cell by cell: for every refined coarse cell the Q1 shape function of each of its 2^dim
                    vertices at each of the 3^dim vertices of its children; boundary columns dropped, an entry set once
                    however many cells reach it.

Both return (P, Pt): namespaces n_rows, n_cols, nnz, rowptr (int64), col (int32), val (float64); the rows of P in ascending
column order, row c of Pt (column c of P) in ascending fine DoF, the header's "ascending source-row order".  All values are
products of 1 and 1/2: exact in fp64.

    apply_reference   P x, or y + Pt r, in numpy.longdouble, with the per-row bound gamma_k sum_j |p_ij x_j|, k the row's
                      entry count (k + 1 and + |y_i| for the add into y), gamma_k = k u / (1 - k u): the form of
                      tests/partition_reference.py.  It holds for every order of the row's sum, with or without fused
                      multiply-adds.
    sequential        the same product summed in fp64 in stored order (what the header promises of the device).

`mistake` seeds one wrong reading of the contract into from_cells for the mutation proofs of
tests/test_transfer_reference_cpu.py; None is the reference."""
import itertools
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -53
FIELD_BITS = 21
SCAN_PASS = 16384

MISTAKES = ("boundary-kept", "weights-3d", "row-by-coordinate", "transpose-by-coordinate", "absent-parent", "key-20-bits", "rowptr-restart")


def _ns(n_rows, n_cols, rowptr, col, val):
    return SimpleNamespace(n_rows=int(n_rows), n_cols=int(n_cols), nnz=int(len(col)), rowptr=np.asarray(rowptr, dtype=np.int64),
                           col=np.asarray(col, dtype=np.int32), val=np.asarray(val, dtype=np.float64))


# ------------------------------------------------------------------------------------------------ A: the definition

def from_vertices(dim, coarse_vertex, coarse_boundary, fine_vertex, fine_spacing, chunk_entries=1 << 22):
    H = 2.0 * float(fine_spacing)
    field = lambda k, d: ((np.asarray(k, dtype=np.uint64) >> np.uint64(21 * d)) & np.uint64(0x1FFFFF)).astype(np.float64)
    xc = [field(coarse_vertex, d) for d in range(dim)]
    xf = [field(fine_vertex, d) for d in range(dim)]
    nc, nf = len(xc[0]), len(xf[0])
    dropped = np.asarray(coarse_boundary) != 0
    step = max(1, chunk_entries // max(nc, 1))
    ii, jj, ww = [], [], []
    for r0 in range(0, nf, step):
        r1 = min(nf, r0 + step)
        W = np.ones((r1 - r0, nc))
        for d in range(dim):
            W *= np.maximum(0.0, 1.0 - np.abs(xf[d][r0:r1, None] - xc[d][None, :]) / H)
        W[:, dropped] = 0.0
        i, j = np.nonzero(W)   # row-major: ascending row, ascending column within a row
        ii.append(i + r0)
        jj.append(j)
        ww.append(W[i, j])
    i, j, w = (np.concatenate(a) for a in (ii, jj, ww))
    P = _ns(nf, nc, np.concatenate([[0], np.cumsum(np.bincount(i, minlength=nf))]), j, w)
    order = np.lexsort((i, j))   # by column, then by fine DoF
    Pt = _ns(nc, nf, np.concatenate([[0], np.cumsum(np.bincount(j, minlength=nc))]), i[order], w[order])
    return P, Pt


# ------------------------------------------------------------------------------------------------ B: cell by cell

def _pack(xyz, bits=FIELD_BITS):
    """x | y << 21 | z << 42 of int64 coordinates [n, 3] (bits < 21: the seeded mistake of a narrower field)"""
    m = np.uint64((1 << bits) - 1)
    x = np.asarray(xyz, dtype=np.int64).astype(np.uint64)
    return (x[:, 0] & m) | ((x[:, 1] & m) << np.uint64(21)) | ((x[:, 2] & m) << np.uint64(42))


class _Table:
    """vertex key -> DoF of one level"""

    def __init__(self, keys, what):
        self.keys = np.asarray(keys, dtype=np.uint64)
        self.order = np.argsort(self.keys, kind="stable")
        self.sorted = self.keys[self.order]
        self.what = what
        if len(self.sorted) > 1 and np.any(self.sorted[1:] == self.sorted[:-1]):
            raise ValueError(f"{what}: a vertex is listed twice")

    def find(self, q):
        """(DoF, found)"""
        at = np.minimum(np.searchsorted(self.sorted, q), max(len(self.sorted) - 1, 0))
        return self.order[at], self.sorted[at] == q


def _rows_of(major, minor, val, n_major, n_minor):
    """CSR of the entries (major, minor) -> val, each pair kept once (its first value: every cell gives the same), rows in
    ascending minor index"""
    code, first = np.unique(major.astype(np.int64) * np.int64(n_minor) + minor.astype(np.int64), return_index=True)
    return _ns(n_major, n_minor, np.searchsorted(code // n_minor, np.arange(n_major + 1)), code % n_minor, val[first])


def from_cells(dim, coarse_vertex, coarse_boundary, fine_vertex, cells, fine_spacing, mistake=None):
    """cells [m, 3]: the lowest vertex of every refined coarse cell, in the units of the keys (z = 0 in 2D)"""
    assert mistake is None or mistake in MISTAKES, mistake
    h = int(fine_spacing)
    bits = 20 if mistake == "key-20-bits" else FIELD_BITS
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    coarse, fine = _Table(coarse_vertex, "coarse level"), _Table(fine_vertex, "fine level")
    nc, nf = len(coarse.keys), len(fine.keys)
    flagged = np.asarray(coarse_boundary) != 0
    ff, cc, ww = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0)]
    for a in itertools.product((0, 1), repeat=dim):          # vertex a of the coarse cell
        corner = cells.copy()
        corner[:, :dim] += 2 * h * np.array(a, dtype=np.int64)
        c, c_found = coarse.find(_pack(corner, bits))
        if mistake is None and not np.all(c_found):
            raise ValueError("a refined cell has a vertex that is no DoF of the coarse level")
        for t in itertools.product((0, 1, 2), repeat=dim):   # vertex t of the 2^dim children, in fine spacings from the cell's lowest
            N = 1.0
            for d in range(dim):
                N *= t[d] / 2.0 if a[d] else 1.0 - t[d] / 2.0
            if mistake == "weights-3d" and dim == 2:
                N *= 0.5   # the z factor of the 3D shape function, taken at the mid-plane of a cell that has none
            if N == 0.0:
                continue
            child = cells.copy()
            child[:, :dim] += h * np.array(t, dtype=np.int64)
            f, f_found = fine.find(_pack(child, bits))
            if mistake is None and not np.all(f_found):
                raise ValueError("a child vertex of a refined cell is no DoF of the fine level")
            keep = f_found & (c_found if mistake != "absent-parent" else True)   # (a mistaken key may miss: no entry)
            if mistake != "boundary-kept":
                keep = keep & ~flagged[c]
            ff.append(f[keep])
            cc.append(c[keep])
            ww.append(np.full(int(np.sum(keep)), N))
    f, c, w = np.concatenate(ff), np.concatenate(cc), np.concatenate(ww)
    P, Pt = _rows_of(f, c, w, nf, nc), _rows_of(c, f, w, nc, nf)
    if mistake == "row-by-coordinate":
        P = _reordered(P, coarse.keys)
    if mistake == "transpose-by-coordinate":
        Pt = _reordered(Pt, fine.keys)
    if mistake == "rowptr-restart":
        for m in (P, Pt):
            m.rowptr = m.rowptr - m.rowptr[(np.arange(m.n_rows + 1) // SCAN_PASS) * SCAN_PASS]
    return P, Pt


def _reordered(m, key_of_col):
    """the seeded mistake of a row sorted by its columns' vertices (z, then y, then x) instead of their DoFs"""
    row = np.repeat(np.arange(m.n_rows), np.diff(m.rowptr))
    order = np.lexsort((key_of_col[m.col], row))
    return _ns(m.n_rows, m.n_cols, m.rowptr, m.col[order], m.val[order])


# ------------------------------------------------------------------------------------------------ comparisons

def same(a, b):
    """array for array"""
    return ((a.n_rows, a.n_cols, a.nnz) == (b.n_rows, b.n_cols, b.nnz) and a.rowptr.dtype == b.rowptr.dtype == np.int64
            and a.col.dtype == b.col.dtype == np.int32 and a.val.dtype == b.val.dtype == np.float64
            and np.array_equal(a.rowptr, b.rowptr) and np.array_equal(a.col, b.col) and np.array_equal(a.val.view(np.uint64), b.val.view(np.uint64)))


# ------------------------------------------------------------------------------------------------ application

def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def apply_reference(m, x, y0=None):
    """(y, bound): y = m x (+ y0) in numpy.longdouble; bound_i = gamma_k sum_j |m_ij x_j| with k the entry count of row i, or
    gamma_(k+1) (|y0_i| + sum_j |m_ij x_j|) with y0"""
    rp = np.asarray(m.rowptr, dtype=np.int64)
    k = np.diff(rp)
    row = np.repeat(np.arange(m.n_rows), k)
    p = np.asarray(m.val, dtype=np.longdouble) * np.asarray(x, dtype=np.longdouble)[np.asarray(m.col, dtype=np.int64)]
    y = np.zeros(m.n_rows, dtype=np.longdouble) if y0 is None else np.array(y0, dtype=np.longdouble)
    t = np.zeros(m.n_rows, dtype=np.longdouble) if y0 is None else np.abs(y)
    np.add.at(y, row, p)
    np.add.at(t, row, np.abs(p))
    return y, gamma(k if y0 is None else k + 1) * t.astype(np.float64)


def sequential(m, x, y0=None):
    """the fp64 sum in stored order, y0 first"""
    y = np.zeros(m.n_rows) if y0 is None else np.array(y0, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    k = np.diff(m.rowptr)
    for q in range(int(k.max()) if len(k) else 0):   # the q-th entry of every row that has one
        rows = np.flatnonzero(k > q)
        at = m.rowptr[rows] + q
        y[rows] = y[rows] + m.val[at] * x[m.col[at]]
    return y


def error_ratio(got, y, bound):
    """max_i |got_i - y_i| / bound_i; a row with bound 0 must be met exactly (ratio 0) or counts as inf"""
    err = np.abs(np.asarray(got, dtype=np.longdouble) - y).astype(np.float64)
    if not np.all(np.isfinite(err)):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if len(r) else 0.0
