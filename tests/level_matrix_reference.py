"""The multigrid level matrix A_l, its Jacobi diagonal and Chebyshev bound, and the interface matrix I_l with its transpose,
restated from the definitions of csrc/gmg_assemble.hpp on the arrays Problem.level_assembly_inputs
exports -- plain loops over dictionaries, no call into the driver:

  A_l pattern  row r stores the sorted union of the DoFs of all cells that contain r (zeros kept);
  A_l values   from +0.0; cells ascending, i ascending: flags[dofs[i]] != 0: (dofs[i], dofs[i]) += |K[i][i]|, nothing else from
               this i; otherwise for j ascending with flags[dofs[j]] == 0: (dofs[i], dofs[j]) += K[i][j];
  invd, lmax   invd[r] = 1 / a_rr (a_rr = 0.0 where the row stores no diagonal); lmax = max_r (sum_k |a_rk| in stored order) /
               |a_rr|, the maximum taken as std::max takes it (a NaN ratio is skipped);
  I_l          pairs (dofs[i], dofs[j]) with flags[dofs[i]] == 2 and flags[dofs[j]] == 0, each the sum of its cells' K[i][j] in
               cell order starting from the first contribution; sums == 0.0 are dropped;
  I_l^T        every column's entries in ascending row.

Python floats are IEEE doubles and a + b rounds once, so the sums carry the bits the sequential host loop produces."""
from types import SimpleNamespace

import numpy as np

BOUNDARY, EDGE = 1, 2


def _csr(n, rows):
    """rows: per row a dict column -> value; columns ascending"""
    rowptr = np.zeros(n + 1, dtype=np.int64)
    col, val = [], []
    for r, row in enumerate(rows):
        for c in sorted(row):
            col.append(c)
            val.append(row[c])
        rowptr[r + 1] = len(col)
    return SimpleNamespace(n_rows=n, n_cols=n, nnz=len(col), rowptr=rowptr, col=np.array(col, dtype=np.int32), val=np.array(val, dtype=np.float64))


def assemble(inp):
    """namespace(A, invd, lmax, I, It): I and It without the dropped zeros (nnz 0: the level has no interface matrix)"""
    n = int(inp.n_dofs)
    cells = np.asarray(inp.cell_dofs).reshape(-1, 1 << int(inp.dim)).tolist()
    K = np.asarray(inp.K, dtype=np.float64).reshape(1 << int(inp.dim), -1).tolist()
    fl = [int(f) for f in np.asarray(inp.dof_flags)]
    A = [dict() for _ in range(n)]
    for dofs in cells:
        for r in dofs:
            for c in dofs:
                A[r].setdefault(c, 0.0)
    I = [dict() for _ in range(n)]
    for dofs in cells:
        for i, r in enumerate(dofs):
            if fl[r] != 0:
                A[r][r] += abs(K[i][i])
                continue
            for j, c in enumerate(dofs):
                if fl[c] == 0:
                    A[r][c] += K[i][j]
        for i, r in enumerate(dofs):
            if fl[r] != EDGE:
                continue
            for j, c in enumerate(dofs):
                if fl[c] == 0:
                    I[r][c] = I[r][c] + K[i][j] if c in I[r] else K[i][j]
    invd, lmax = np.zeros(n), 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for r in range(n):
            aii, rs = np.float64(0.0), 0.0
            for c in sorted(A[r]):
                if c == r:
                    aii = np.float64(A[r][c])
                rs += abs(A[r][c])
            invd[r] = np.float64(1.0) / aii
            ratio = float(np.float64(rs) / abs(aii))
            if lmax < ratio:
                lmax = ratio
    kept = [{c: v for c, v in row.items() if v != 0.0} for row in I]
    T = [dict() for _ in range(n)]
    for r, row in enumerate(kept):
        for c, v in row.items():
            T[c][r] = v
    return SimpleNamespace(A=_csr(n, A), invd=invd, lmax=lmax, I=_csr(n, kept), It=_csr(n, T))


def pruned(m):
    """a CSR without its stored zeros (what gmg_set_edge_matrix keeps of the host's I_l); None or an empty matrix: no entries"""
    if m is None or m.n_rows == 0:
        return None
    keep = np.asarray(m.val) != 0.0
    rows = np.repeat(np.arange(m.n_rows), np.diff(m.rowptr))[keep]
    rowptr = np.zeros(m.n_rows + 1, dtype=np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return SimpleNamespace(n_rows=m.n_rows, n_cols=m.n_cols, nnz=int(keep.sum()), rowptr=np.cumsum(rowptr), col=np.asarray(m.col)[keep],
                           val=np.asarray(m.val)[keep])


def transposed(m):
    """the stable transpose: every column's entries in ascending row"""
    rows = np.repeat(np.arange(m.n_rows), np.diff(m.rowptr))
    order = np.argsort(np.asarray(m.col), kind="stable")
    rowptr = np.zeros(m.n_cols + 1, dtype=np.int64)
    np.add.at(rowptr, np.asarray(m.col, dtype=np.int64) + 1, 1)
    return SimpleNamespace(n_rows=m.n_cols, n_cols=m.n_rows, nnz=m.nnz, rowptr=np.cumsum(rowptr), col=rows[order].astype(np.int32),
                           val=np.asarray(m.val)[order])


def same_bits(a, b):
    """two CSR matrices with identical pattern and values identical as bit patterns"""
    return (a.n_rows == b.n_rows and np.array_equal(np.asarray(a.rowptr, dtype=np.int64), np.asarray(b.rowptr, dtype=np.int64))
            and np.array_equal(np.asarray(a.col, dtype=np.int32), np.asarray(b.col, dtype=np.int32))
            and np.array_equal(np.asarray(a.val, dtype=np.float64).view(np.uint64), np.asarray(b.val, dtype=np.float64).view(np.uint64)))


def same_or_absent(dev, ref):
    """an interface matrix against its reference, where either may be absent (None, no rows, or no entries)"""
    if ref is None or ref.nnz == 0:
        return dev is None or dev.nnz == 0
    return dev is not None and same_bits(dev, ref)


# ------------------------------------------------------------------------------------------------ hand-built 2D inputs

K2D = np.array([[4.0, -1.0, -1.0, -2.0], [-1.0, 4.0, -2.0, -1.0], [-1.0, -2.0, 4.0, -1.0], [-2.0, -1.0, -1.0, 4.0]]) / 6.0


def patch_2d():
    """3 x 3 cells on 4 x 4 vertices (lexicographic) with mixed flags: the outer ring is boundary except the top row, which is
    on the refinement edge (its corners are both), the interior is free -- boundary rows, edge rows with entries of I_l into
    the two free vertices below them, and an edge + boundary corner that has none.  K[2][1] is an exact zero: the pair (13, 10)
    has that one contribution, so I_l drops it."""
    cells = [[v, v + 1, v + 4, v + 5] for y in range(3) for v in (4 * y + x for x in range(3))]
    fl = np.zeros(16, dtype=np.uint8)
    for v in range(16):
        x, y = v % 4, v // 4
        if x in (0, 3) or y == 0:
            fl[v] |= BOUNDARY
        if y == 3:
            fl[v] |= EDGE
    K = K2D.copy()
    K[2][1] = 0.0
    return SimpleNamespace(dim=2, n_dofs=16, cell_dofs=np.array(cells, dtype=np.int32), K=K, dof_flags=fl)


def fan_2d(n_cells):
    """n_cells cells that all hold DoF 0 and three DoFs of their own: row 0 has 3 n_cells + 1 columns.  DoF 0 is on the
    refinement edge, every third cell has a boundary DoF, the rest is free."""
    cells = [[0, 3 * c + 1, 3 * c + 2, 3 * c + 3] for c in range(n_cells)]
    fl = np.zeros(3 * n_cells + 1, dtype=np.uint8)
    fl[0] = EDGE
    fl[3::9] = BOUNDARY
    return SimpleNamespace(dim=2, n_dofs=3 * n_cells + 1, cell_dofs=np.array(cells, dtype=np.int32), K=K2D.copy(), dof_flags=fl)
