"""An independent restatement of the active-mesh system matrix (include/gmg_coulomb.h, gmg_assemble_system_matrix) in numpy,
from the exported input arrays alone: cell DoFs, cell levels, the per-level cell matrix and the constraint lines.  It shares
no code with the host driver or the kernels.

Pattern: a cell's coupling list is its DoFs plus the masters of its constrained DoFs; every ordered pair of one list is a
stored entry; rows hold their columns ascending.

Values: every contribution of the sequential loop is generated as one array element whose position in C order IS the loop's
order -- [cell][i][slot] with slot 0 the |K[i][i]| a constrained i adds to its own diagonal before its j loop and slot
1 + (j * M + ri) * M + rj the pair (ri, rj) of vertices (i, j), M the longest line (an unconstrained vertex has the one
"entry" (itself, no weight)) -- and added with numpy.add.at, which is unbuffered and adds element after element.  The
products are single fp64 multiplications: w * K, or (w_i * w_j) * K for a doubly constrained pair."""
from types import SimpleNamespace

import numpy as np

CHUNK = 2048  # cells per block of generated contributions


def _targets(inp):
    """per (cell, vertex): up to M (row, weight) targets, whether each exists, and whether the vertex is constrained"""
    cd = np.asarray(inp.cell_dofs, dtype=np.int64)
    lp = np.asarray(inp.line_ptr, dtype=np.int64)
    lm = np.asarray(inp.line_master, dtype=np.int64)
    lw = np.asarray(inp.line_weight, dtype=np.float64)
    cons = np.asarray(inp.constraint_of_dof, dtype=np.int64)
    line = cons[cd] if cd.size else np.zeros(cd.shape, dtype=np.int64)
    constrained = line >= 0
    ln = np.where(constrained, line, 0)
    length = np.where(constrained, lp[ln + 1] - lp[ln], 1) if lp.size > 1 else np.ones(cd.shape, dtype=np.int64)
    M = int(max(1, (lp[1:] - lp[:-1]).max() if lp.size > 1 else 1))
    k = np.arange(M)
    exists = k < length[..., None]
    if lm.size:
        e = np.minimum(np.where(constrained, lp[ln] if lp.size > 1 else 0, 0)[..., None] + k, lm.size - 1)
        row = np.where(constrained[..., None], lm[e], cd[..., None])
        w = np.where(constrained[..., None], lw[e], 1.0)
    else:
        row = np.broadcast_to(cd[..., None], cd.shape + (M,)).copy()
        w = np.ones(cd.shape + (M,))
    return row, w, exists, constrained, M


def pattern(inp):
    """(rowptr, col) and the sorted keys row * n + col of the stored entries"""
    n = int(inp.n_dofs)
    cd = np.asarray(inp.cell_dofs, dtype=np.int64)
    nc = cd.shape[0]
    keys = np.zeros(0, dtype=np.int64)
    if nc:
        row, _, exists, constrained, M = _targets(inp)
        nv = cd.shape[1]
        # the coupling list: the DoFs, and the masters of the constrained ones
        members = np.concatenate([cd, row.reshape(nc, nv * M)], axis=1)
        valid = np.concatenate([np.ones_like(cd, dtype=bool), (exists & constrained[..., None]).reshape(nc, nv * M)], axis=1)
        parts = []
        for c0 in range(0, nc, CHUNK):
            m, v = members[c0:c0 + CHUNK], valid[c0:c0 + CHUNK]
            kk = m[:, :, None] * n + m[:, None, :]
            parts.append(np.unique(kk[v[:, :, None] & v[:, None, :]]))
        keys = np.unique(np.concatenate(parts))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, keys // max(n, 1) + 1, 1)
    return np.cumsum(rowptr), (keys % max(n, 1)).astype(np.int32), keys


def assemble(inp):
    """the CSR of the system matrix: namespace(n_rows, n_cols, nnz, rowptr, col, val)"""
    n = int(inp.n_dofs)
    rowptr, col, keys = pattern(inp)
    val = np.zeros(len(keys))
    cd = np.asarray(inp.cell_dofs, dtype=np.int64)
    nc = cd.shape[0]
    if nc:
        nv = cd.shape[1]
        row, w, exists, constrained, M = _targets(inp)
        K = np.asarray(inp.K_of_level, dtype=np.float64).reshape(16, nv, nv)[np.asarray(inp.cell_level, dtype=np.int64)]
        line_empty = constrained & ~exists[..., 0]  # a line without entries: its pairs are skipped
        for c0 in range(0, nc, CHUNK):
            s = slice(c0, c0 + CHUNK)
            r_, w_, ex, con, Kc, d_ = row[s], w[s], exists[s], constrained[s], K[s], cd[s]
            b = r_.shape[0]
            # [cell, i, j, ri, rj]
            ri = np.broadcast_to(r_[:, :, None, :, None], (b, nv, nv, M, M))
            rj = np.broadcast_to(r_[:, None, :, None, :], (b, nv, nv, M, M))
            wi, wj = w_[:, :, None, :, None], w_[:, None, :, None, :]
            ci, cj = con[:, :, None, None, None], con[:, None, :, None, None]
            kij = Kc[:, :, :, None, None]
            value = np.where(ci & cj, (wi * wj) * kij, np.where(ci, wi * kij, np.where(cj, wj * kij, kij)))
            ok = ex[:, :, None, :, None] & ex[:, None, :, None, :]
            skip = line_empty[s]
            ok = ok & ~skip[:, :, None, None, None] & ~skip[:, None, :, None, None]
            pair_keys = (ri * n + rj).reshape(b, nv, nv * M * M)
            pair_vals = np.broadcast_to(value, (b, nv, nv, M, M)).reshape(b, nv, nv * M * M)
            pair_ok = ok.reshape(b, nv, nv * M * M)
            # slot 0 of every (cell, i): the diagonal of a constrained row
            diag = np.abs(Kc[:, np.arange(nv), np.arange(nv)])
            all_keys = np.concatenate([(d_ * n + d_)[..., None], pair_keys], axis=2).reshape(-1)
            all_vals = np.concatenate([diag[..., None], pair_vals], axis=2).reshape(-1)
            all_ok = np.concatenate([con[..., None], pair_ok], axis=2).reshape(-1)
            pos = np.searchsorted(keys, all_keys[all_ok])
            assert np.array_equal(keys[pos], all_keys[all_ok]), "a contribution outside the pattern"
            np.add.at(val, pos, all_vals[all_ok])
    return SimpleNamespace(n_rows=n, n_cols=n, nnz=len(keys), rowptr=rowptr, col=col, val=val)


def assemble_loops(inp):
    """the same in plain Python loops over dictionaries (small meshes: a check of the array formulation above)"""
    n, cd = int(inp.n_dofs), np.asarray(inp.cell_dofs)
    nv = cd.shape[1] if cd.size else 1
    K = np.asarray(inp.K_of_level, dtype=np.float64).reshape(16, nv, nv)
    lines = [[(int(inp.line_master[e]), float(inp.line_weight[e])) for e in range(int(inp.line_ptr[l]), int(inp.line_ptr[l + 1]))]
             for l in range(len(inp.line_ptr) - 1)]
    entries = {}
    for c in range(cd.shape[0]):
        members = set()
        for a in range(nv):
            members.add(int(cd[c, a]))
            if inp.constraint_of_dof[cd[c, a]] >= 0:
                members.update(m for m, _ in lines[inp.constraint_of_dof[cd[c, a]]])
        for r in members:
            for q in members:
                entries.setdefault((r, q), 0.0)
    for c in range(cd.shape[0]):
        Kc = K[int(inp.cell_level[c])]
        d = [int(v) for v in cd[c]]
        ln = [lines[inp.constraint_of_dof[v]] if inp.constraint_of_dof[v] >= 0 else None for v in d]
        for i in range(nv):
            if ln[i] is not None:
                entries[(d[i], d[i])] += abs(float(Kc[i, i]))
            for j in range(nv):
                k = float(Kc[i, j])
                if ln[i] is None and ln[j] is None:
                    entries[(d[i], d[j])] += k
                elif (ln[i] is not None and not ln[i]) or (ln[j] is not None and not ln[j]):
                    continue
                elif ln[i] is not None and ln[j] is not None:
                    for mi, wi in ln[i]:
                        for mj, wj in ln[j]:
                            entries[(mi, mj)] += (wi * wj) * k
                elif ln[i] is not None:
                    for mi, wi in ln[i]:
                        entries[(mi, d[j])] += wi * k
                else:
                    for mj, wj in ln[j]:
                        entries[(d[i], mj)] += wj * k
    keys = sorted(entries)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    for r, _ in keys:
        rowptr[r + 1] += 1
    return SimpleNamespace(n_rows=n, n_cols=n, nnz=len(keys), rowptr=np.cumsum(rowptr), col=np.array([q for _, q in keys], dtype=np.int32),
                           val=np.array([entries[k] for k in keys], dtype=np.float64))


def same_bits(a, b):
    """two CSR matrices with identical pattern and values identical as bit patterns"""
    return (a.n_rows == b.n_rows and np.array_equal(np.asarray(a.rowptr, dtype=np.int64), np.asarray(b.rowptr, dtype=np.int64))
            and np.array_equal(np.asarray(a.col, dtype=np.int32), np.asarray(b.col, dtype=np.int32))
            and np.array_equal(np.asarray(a.val, dtype=np.float64).view(np.uint64), np.asarray(b.val, dtype=np.float64).view(np.uint64)))


def quadrant_mesh_2d():
    """A hand-built 2D mesh: a square of 3 x 3 cells whose bottom middle cell is cut in four.  12 active cells (8 on level 1,
    4 on level 2), 21 vertices.  The refined cell shares three edges with coarse neighbours, so three vertices hang: the
    midpoints of its left and right edges, whose second master lies on the boundary (the resolved lines keep the interior
    master alone, weight 0.5), and the midpoint of its top edge (two interior masters, 0.5 each).  Boundary DoFs are on
    Dirichlet lines without entries.  Returns the inputs of gmg_assemble_system_matrix (dim 2, K the Q1 Laplacian, which
    in 2D is the same on every level)."""
    pts = {}

    def dof(x, y):  # coordinates in halves of a coarse cell
        return pts.setdefault((x, y), len(pts))

    cells, levels = [], []

    def cell(x, y, h, level):
        cells.append([dof(x, y), dof(x + h, y), dof(x, y + h), dof(x + h, y + h)])
        levels.append(level)

    for y in (0, 2, 4):
        for x in (0, 2, 4):
            if (x, y) != (2, 0):
                cell(x, y, 2, 1)
    for x, y in ((2, 0), (3, 0), (2, 1), (3, 1)):
        cell(x, y, 1, 2)
    n = len(pts)
    cons = -np.ones(n, dtype=np.int32)
    line_ptr, master, weight = [0], [], []

    def add_line(d, ent):
        cons[d] = len(line_ptr) - 1
        for m, w in ent:
            master.append(m)
            weight.append(w)
        line_ptr.append(len(master))

    for (x, y), d in sorted(pts.items(), key=lambda t: t[1]):
        if x in (0, 6) or y in (0, 6):
            add_line(d, [])  # Dirichlet
    add_line(pts[(2, 1)], [(pts[(2, 2)], 0.5)])
    add_line(pts[(4, 1)], [(pts[(4, 2)], 0.5)])
    add_line(pts[(3, 2)], [(pts[(2, 2)], 0.5), (pts[(4, 2)], 0.5)])
    K1 = np.array([[4, -1, -1, -2], [-1, 4, -2, -1], [-1, -2, 4, -1], [-2, -1, -1, 4]], dtype=np.float64) / 6.0
    return SimpleNamespace(dim=2, n_dofs=n, cell_dofs=np.array(cells, dtype=np.int32), cell_level=np.array(levels, dtype=np.uint8),
                           K_of_level=np.broadcast_to(K1, (16, 4, 4)).copy(), constraint_of_dof=cons,
                           line_ptr=np.array(line_ptr, dtype=np.int64), line_master=np.array(master, dtype=np.int32),
                           line_weight=np.array(weight, dtype=np.float64))
