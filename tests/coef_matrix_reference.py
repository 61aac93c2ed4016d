"""The operators of a variable coefficient restated from the definitions of include/gmg_coulomb.h
(gmg_assemble_system_matrix_coef, gmg_assemble_level_matrix_coef) on the arrays
Problem.system_coefficient_inputs() / Problem.level_coefficient_inputs(level) export -- no call into the driver's assembly:

  K_c          K_c[i][j] = +0.0; for q ascending: K_c[i][j] += ((cell_coef[c][q] * G[q][i][j]) * qw[q]) * scale
               (scale = scale_of_level[cell_level[c]] for the system matrix, the level's one scale for A_l);
  system       the pattern and the sums of gmg_assemble_system_matrix with K_c in place of K[level];
  A_l, I_l     the patterns and the sums of gmg_assemble_level_matrix with K_c in place of K; invd, lmax, I_l without its
               zeros, I_l^T.

Every product and every sum is one fp64 operation that rounds once (numpy element by element, or Python floats), in the order
of the definition, so the results carry the bits of the sequential host loop."""
from types import SimpleNamespace

import numpy as np

from level_matrix_reference import pruned, same_bits, same_or_absent, transposed  # noqa: F401  (for the tests)

EDGE = 2


def cell_matrices(nq, cell_coef, G, qw, scale):
    """K_c of every cell, [n_cells, nv, nv]: the loop over q is the definition's, every cell and (i, j) an array element.
    scale: one value per cell."""
    G = np.asarray(G, dtype=np.float64)
    nv = G.shape[-1]
    G = G.reshape(nq, nv, nv)
    cc = np.asarray(cell_coef, dtype=np.float64).reshape(-1, nq)
    w = np.asarray(qw, dtype=np.float64).reshape(nq)
    s = np.asarray(scale, dtype=np.float64).reshape(-1, 1, 1)
    K = np.zeros((cc.shape[0], nv, nv))
    for q in range(nq):
        K = K + ((cc[:, q, None, None] * G[q][None, :, :]) * w[q]) * s
    return K


def cell_matrix_loops(nq, coef, G, qw, scale):
    """one K_c in plain Python floats (a check of the array form above)"""
    G = np.asarray(G, dtype=np.float64)
    nv = G.shape[-1]
    g, w, c = G.reshape(nq, nv, nv).tolist(), [float(v) for v in qw], [float(v) for v in coef]
    K = [[0.0] * nv for _ in range(nv)]
    for i in range(nv):
        for j in range(nv):
            for q in range(nq):
                K[i][j] += ((c[q] * g[q][i][j]) * w[q]) * float(scale)
    return np.array(K)


def system_cell_matrices(inp):
    return cell_matrices(inp.nq, inp.cell_coef, inp.G, inp.qw, np.asarray(inp.scale_of_level, dtype=np.float64)[np.asarray(inp.cell_level, dtype=np.int64)])


def level_cell_matrices(inp):
    n_cells = np.asarray(inp.cell_dofs).reshape(-1, 1 << int(inp.dim)).shape[0]
    return cell_matrices(inp.nq, inp.cell_coef, inp.G, inp.qw, np.full(n_cells, float(inp.scale)))


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


def assemble_system(inp):
    """the CSR of the system matrix: namespace(n_rows, n_cols, nnz, rowptr, col, val)"""
    n = int(inp.n_dofs)
    nv = 1 << int(inp.dim)
    cd = np.asarray(inp.cell_dofs).reshape(-1, nv).tolist()
    K = system_cell_matrices(inp).tolist()
    cons = [int(v) for v in np.asarray(inp.constraint_of_dof)]
    lp = [] if inp.line_ptr is None else [int(v) for v in inp.line_ptr]
    lines = [[(int(inp.line_master[e]), float(inp.line_weight[e])) for e in range(lp[l], lp[l + 1])] for l in range(len(lp) - 1)]
    A = [dict() for _ in range(n)]
    for d in cd:
        members = set(d)
        for v in d:
            if cons[v] >= 0:
                members.update(m for m, _ in lines[cons[v]])
        for r in members:
            for q in members:
                A[r].setdefault(q, 0.0)
    for d, Kc in zip(cd, K):
        ln = [lines[cons[v]] if cons[v] >= 0 else None for v in d]
        for i in range(nv):
            if ln[i] is not None:
                A[d[i]][d[i]] += abs(Kc[i][i])
            for j in range(nv):
                k = Kc[i][j]
                if ln[i] is None and ln[j] is None:
                    A[d[i]][d[j]] += k
                elif (ln[i] is not None and not ln[i]) or (ln[j] is not None and not ln[j]):
                    continue
                elif ln[i] is not None and ln[j] is not None:
                    for mi, wi in ln[i]:
                        for mj, wj in ln[j]:
                            A[mi][mj] += (wi * wj) * k
                elif ln[i] is not None:
                    for mi, wi in ln[i]:
                        A[mi][d[j]] += wi * k
                else:
                    for mj, wj in ln[j]:
                        A[d[i]][mj] += wj * k
    return _csr(n, A)


def assemble_level(inp):
    """namespace(A, invd, lmax, I, It): I and It without the dropped zeros (nnz 0: the level has no interface matrix)"""
    n = int(inp.n_dofs)
    nv = 1 << int(inp.dim)
    cells = np.asarray(inp.cell_dofs).reshape(-1, nv).tolist()
    K = level_cell_matrices(inp).tolist()
    fl = [int(f) for f in np.asarray(inp.dof_flags)]
    A = [dict() for _ in range(n)]
    for dofs in cells:
        for r in dofs:
            for c in dofs:
                A[r].setdefault(c, 0.0)
    I = [dict() for _ in range(n)]
    for dofs, Kc in zip(cells, K):
        for i, r in enumerate(dofs):
            if fl[r] != 0:
                A[r][r] += abs(Kc[i][i])
                continue
            for j, c in enumerate(dofs):
                if fl[c] == 0:
                    A[r][c] += Kc[i][j]
        for i, r in enumerate(dofs):
            if fl[r] != EDGE:
                continue
            for j, c in enumerate(dofs):
                if fl[c] == 0:
                    I[r][c] = I[r][c] + Kc[i][j] if c in I[r] else Kc[i][j]
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


# ------------------------------------------------------------------------------------------------ inputs made by hand

def with_coefficients(inp, nq, cell_coef, G, qw, **scale):
    """the inputs `inp` of a cell-matrix entry turned into those of its coefficient form (K / K_of_level dropped)"""
    d = {k: v for k, v in vars(inp).items() if k not in ("K", "K_of_level")}
    d.update(nq=int(nq), cell_coef=np.asarray(cell_coef, dtype=np.float64), G=np.asarray(G, dtype=np.float64), qw=np.asarray(qw, dtype=np.float64), **scale)
    return SimpleNamespace(**d)


def random_coefficients(rng, n_cells, nq):
    """values in [0.25, 8), about 5 % of them negated (a negative K_c[i][i] pins the fabs of a constrained diagonal)"""
    c = rng.uniform(0.25, 8.0, (n_cells, nq))
    return np.where(rng.random((n_cells, nq)) < 0.05, -c, c)


def random_tables(rng, nq, nv):
    """synthetic G [nq, nv, nv] and qw [nq]: nothing symmetric, nothing that depends on nq == nv"""
    return rng.uniform(-1.0, 1.0, (nq, nv, nv)), rng.uniform(0.05, 1.0, nq)
