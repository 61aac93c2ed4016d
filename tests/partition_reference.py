"""The row partition and the halo plans of the one-process-per-GPU layout, restated in plain numpy from the documented layout
(include/gmg_coulomb.h, "distributed").  It shares no text with csrc/host/partition.h.

    owned_range(n, rank, N)   rank r owns the rows [r c, (r + 1) c) cut at n, c = ceil(n / N): equal chunks, the last ranks
                              may own fewer rows or none
    localize(csr, rank, N)    the owned rows of a square operator with its columns renumbered [owned | ghosts]: an owned
                              column j becomes j - begin, a ghost column n_owned + its position in ghost_global.  ghost_global
                              lists the off-rank columns the owned rows refer to, grouped by owning rank, ascending global
                              index inside a group (equal chunks: that is plain ascending order).  The halo plan names, per
                              neighbour, the owned local rows to send (send_idx, neighbour after neighbour) and the number of
                              ghost values received; ghosts sit behind the owned entries in neighbour order.

What the header leaves open and the host code (Problem.localize, the code production runs) fixes; this file follows it:
    * neighbours are listed in ascending rank;
    * a rank is a neighbour when either count of the pair is nonzero (an operator whose pattern is not symmetric has pairs
      with one count of zero: the rank that only sends still lists the receiver, with recv_count 0);
    * send_idx of one neighbour is in ascending local index, which is the order of that neighbour's ghost segment;
    * a row keeps its entries in their stored order: the columns are renumbered in place, not sorted again, so a row's
      local columns are not ascending where a ghost of a lower rank stands before an owned column.
Everything else is fixed by the layout, and a disagreement with the host code there is a finding."""
from types import SimpleNamespace

import numpy as np


def chunk(n, n_ranks):
    return -(-int(n) // int(n_ranks))


def owned_range(n, rank, n_ranks):
    c = chunk(n, n_ranks)
    return min(int(n), rank * c), min(int(n), (rank + 1) * c)


def localize(m, rank, n_ranks):
    n = int(m.n_rows)
    assert int(m.n_cols) == n
    rp = np.asarray(m.rowptr, dtype=np.int64)
    col = np.asarray(m.col, dtype=np.int64)
    val = np.asarray(m.val, dtype=np.float64)
    c = max(chunk(n, n_ranks), 1)
    begin, end = owned_range(n, rank, n_ranks)
    n_owned = end - begin
    row_owner = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp)) // c
    col_owner = col // c
    away = row_owner != col_owner
    # what I need from the others, and what each of the others needs from me
    ghost_global = np.unique(col[away & (row_owner == rank)])
    ghost_owner = ghost_global // c
    neighbor_rank, send_count, recv_count, send_idx = [], [], [], []
    for s in range(n_ranks):
        if s == rank:
            continue
        wanted = np.unique(col[away & (row_owner == s) & (col_owner == rank)]) - begin
        n_recv = int(np.sum(ghost_owner == s))
        if len(wanted) == 0 and n_recv == 0:
            continue
        neighbor_rank.append(s)
        send_count.append(len(wanted))
        recv_count.append(n_recv)
        send_idx.append(wanted)
    k0, k1 = int(rp[begin]), int(rp[end])
    mine = col[k0:k1]
    local = np.where((mine >= begin) & (mine < end), mine - begin, n_owned + np.searchsorted(ghost_global, mine))
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    return SimpleNamespace(n_rows=n_owned, n_cols=n_owned + len(ghost_global), rowptr=rp[begin:end + 1] - k0, col=i32(local),
                           val=val[k0:k1].copy(), nnz=k1 - k0, row_begin=begin, neighbor_rank=i32(neighbor_rank),
                           send_count=i32(send_count), recv_count=i32(recv_count),
                           send_idx=i32(np.concatenate(send_idx) if send_idx else []), ghost_global=ghost_global.astype(np.int64))


# ------------------------------------------------------------------------------------------------ the ranks emulated in numpy

def local_vector(loc, x):
    """[owned | ghost tail filled from ghost_global] of the global vector x"""
    return np.concatenate([x[loc.row_begin:loc.row_begin + loc.n_rows], x[loc.ghost_global]])


def segments(loc):
    """(first, last + 1) of every neighbour's segment of the ghost tail, relative to the tail"""
    ends = np.cumsum(loc.recv_count, dtype=np.int64)
    return [(int(e - k), int(e)) for e, k in zip(ends, loc.recv_count)]


def row_sums(m, x):
    """(y, t): y_i = sum_j a_ij x_j and t_i = sum_j |a_ij x_j| in numpy.longdouble"""
    rp = np.asarray(m.rowptr, dtype=np.int64)
    row = np.repeat(np.arange(m.n_rows), np.diff(rp))
    p = np.asarray(m.val, dtype=np.longdouble) * np.asarray(x, dtype=np.longdouble)[np.asarray(m.col, dtype=np.int64)]
    y, t = np.zeros(m.n_rows, dtype=np.longdouble), np.zeros(m.n_rows, dtype=np.longdouble)
    np.add.at(y, row, p)
    np.add.at(t, row, np.abs(p))
    return y, t


U = 2.0 ** -53


def gamma(k):
    """gamma_k = k u / (1 - k u): the bound on the relative error of a sum of k roundings"""
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def spmv_bound(m, x):
    """(y in longdouble, per-row bound gamma_(k+1) sum_j |a_ij x_j|, k the row's length).  The bound holds for any order of the
    row's k products and k - 1 additions, with or without fused multiply-adds."""
    y, t = row_sums(m, x)
    k = np.diff(np.asarray(m.rowptr, dtype=np.int64))
    return y, gamma(k + 1) * t.astype(np.float64)
