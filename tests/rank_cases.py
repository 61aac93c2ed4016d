"""The operators, vectors and step lists of the rank-parallel tests.  tests/rank_worker.py runs the steps
of a group on one rank, tests/test_gpu_ranks_reference.py checks what the ranks wrote, tests/test_partition_reference_cpu.py and
tests/test_cg_reference_cpu.py prove the cases on the CPU: all read this one table.  numpy only: a rank imports neither torch
nor the oracle."""
import functools
from types import SimpleNamespace

import numpy as np

import cg_reference as R

RANKS = (2, 3, 4)
SYSTEM = -1
JACOBI, SSOR, CHEBYSHEV = 0, 1, 2


# ------------------------------------------------------------------------------------------------ operators

def _block_pair(m):
    """two decoupled copies of the tridiagonal operator of m rows: on two ranks the cut falls exactly between them"""
    a = R.tridiagonal_operator(m)
    rp = np.concatenate([a.rowptr, a.rowptr[1:] + a.nnz])
    return SimpleNamespace(n_rows=2 * m, n_cols=2 * m, rowptr=rp, col=np.concatenate([a.col, a.col + m]).astype(np.int32),
                           val=np.concatenate([a.val, a.val]), nnz=2 * a.nnz)


def _one_sided(n):
    """upper triangular pattern: row i refers to i, i + 1 and i + 7.  A rank needs values of the next rank alone, so the last
    rank sends and receives nothing, the first receives and sends nothing"""
    i = np.arange(n, dtype=np.int64)
    ok = np.stack([np.ones(n, bool), i + 1 < n, i + 7 < n], axis=1)
    col = np.stack([i, np.minimum(i + 1, n - 1), np.minimum(i + 7, n - 1)], axis=1)
    val = np.stack([3.0 + np.sin(0.3 * i), -1.0 - 0.5 * np.cos(0.9 * i), 0.5 + 0.25 * np.sin(1.7 * i)], axis=1)
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(ok.sum(axis=1))
    return SimpleNamespace(n_rows=n, n_cols=n, rowptr=rp, col=col[ok].astype(np.int32), val=val[ok], nnz=int(rp[-1]))


WIDE_ROWS = 241     # four ranks: chunks of 61, 61, 61 and 58 rows, couplings up to 120 rows away
BLOCK_ROWS = 129    # per block


@functools.lru_cache(maxsize=None)
def operator(name):
    if name == "wide":      # a band wider than a chunk: non-adjacent neighbours
        return R.banded_operator(WIDE_ROWS, 4, seed=11, period=2, reach=60)
    if name == "blocks":
        return _block_pair(BLOCK_ROWS)
    if name == "unsym":
        return _one_sided(601)
    return R.operator(name)[0]


SPMV_OPERATORS = ("tri1031", "csr", "blocks", "wide", "unsym")   # "blocks" on two ranks only
N_SPMV_VECTORS = 5


def spmv_operators(n_ranks):
    return [o for o in SPMV_OPERATORS if o != "blocks" or n_ranks == 2]


def spmv_cases():
    return [(name, n) for n in RANKS for name in spmv_operators(n)]


@functools.lru_cache(maxsize=None)
def spmv_vectors(name):
    """[N_SPMV_VECTORS, n]: entries of mixed sign, magnitudes over four decades"""
    n = operator(name).n_rows
    rng = np.random.default_rng(sum(name.encode()) + n)
    v = rng.standard_normal((N_SPMV_VECTORS, n)) * 10.0 ** rng.uniform(-2, 2, (N_SPMV_VECTORS, n))
    v.setflags(write=False)
    return v


# ------------------------------------------------------------------------------------------------ coarse CG

COARSE_OPERATORS = ("csr", "band9", "tri257", "blocks", "wide")  # "blocks" on two ranks only
COARSE_KS = {"csr": (1, 7, 8, 9, 15, 16, 17), "band9": (1, 7, 8, 9, 15, 16, 17), "tri257": (1, 7, 8, 9, 15, 16, 17),
             "blocks": (1, 7, 8, 9, 15, 16, 17), "wide": (1, 7, 8, 9, 15, 16, 17)}
COARSE_CHUNKS = (0, 1, 3)
RHS_SEED = {"wide": 8, "blocks": 9}


def coarse_operators(n_ranks):
    return [o for o in COARSE_OPERATORS if o != "blocks" or n_ranks == 2]


@functools.lru_cache(maxsize=None)
def rhs(name):
    if name in RHS_SEED:
        return np.random.default_rng(RHS_SEED[name]).standard_normal(operator(name).n_rows)
    return R.rhs(name)


@functools.lru_cache(maxsize=None)
def _history(name):
    return R.cg(operator(name), rhs(name), 0.0, 40, keep_steps=False).history


@functools.lru_cache(maxsize=None)
def stop_case(name, k, tier="seq"):
    """cg_reference.stop_case for the operators of this file as well: (tol, result)"""
    if name not in RHS_SEED:
        return R.stop_case(name, k, tier=tier)
    tol = R.target_tol(_history(name), k)
    return tol, R.cg(operator(name), rhs(name), tol, 1000, tier=tier)


@functools.lru_cache(maxsize=None)
def refused_case(name, max_it, tier="seq"):
    if name not in RHS_SEED:
        return R.refused_case(name, max_it, tier=tier)
    return R.REFUSE_TOL, R.cg(operator(name), rhs(name), R.REFUSE_TOL, max_it, tier=tier)


def x_tolerance(name):
    """cg_reference.x_tolerance: none of the operators here is one of its large ones"""
    assert operator(name).n_rows < R.LARGE_ROWS
    return R.x_tolerance("csr")


def coarse_pairs():
    """every (operator, k) the ranks solve and tests/cg_reference.gpu_cases() does not hold yet"""
    have = {(c[1], c[2]) for c in R.gpu_cases() if c[0] == "stop" and c[3:] == ("identity", "zero")}
    return [(name, k) for name in COARSE_OPERATORS for k in COARSE_KS[name] if (name, k) not in have]


# ------------------------------------------------------------------------------------------------ collectives

def allgather_sizes(n_ranks):
    return (70001, 1, 4097, n_ranks - 1, n_ranks + 1, n_ranks)   # a long message first, then a short one


def allgather_rounds(n_ranks):
    """lists of n_global, each list enqueued back to back on one context: six rounds of every size (both payload parities and
    the acknowledgement of round seq - 2), then the sizes mixed"""
    n = n_ranks
    return [(s,) * 6 for s in allgather_sizes(n)] + [(70001, 1, 4097, n - 1, 70001, n + 1, n, 1)]


def allgather_values(tag, n_global):
    """entry g of round `tag` (a number that differs from round to round): exact in fp64"""
    return (tag + 1) * 1048576.0 + np.arange(n_global, dtype=np.float64)


REDUCE_LENGTHS = (1, 257, 70001)   # per rank


def reduce_vectors(length, rank):
    rng = np.random.default_rng(100000 * rank + length)
    x = rng.standard_normal(length) * 10.0 ** rng.uniform(-3, 3, length)
    y = rng.standard_normal(length) * 10.0 ** rng.uniform(-3, 3, length)
    return x, y


MIX_OPERATOR = "tri1031"
MIX_OPS = ("halo", "dot", "allgather", "norms") * 5     # 20 collectives on one context, sharing round counter and slots
MIX_GATHER = 4097


def mix_vector(i, n):
    rng = np.random.default_rng(7000 + i)
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2, n)


# ------------------------------------------------------------------------------------------------ outer CG

OUTER_CASES = [(pc, what) for pc in ("identity", "jacobi") for what in ("zero", "random", "converged", "b0", "max_it")]
OUTER_RANKS = (2, 3)


# ------------------------------------------------------------------------------------------------ smoother and V-cycle

MG_RANKS = (2, 3)
MG_HIERARCHIES = ("A3", "B3")
MG_STEPS = (1, 2, 3)


def given_bounds(n_ranks, n):
    """caller-given partitions of n_ranks blocks: an empty block and a block of a single row (two blocks cannot have both
    and cover n rows: two partitions there)"""
    if n_ranks == 2:
        return [(0, 0, n), (0, 1, n)]
    return [(0, 0, 1) + tuple(n * b // (n_ranks - 2) for b in range(1, n_ranks - 1))]


def block_keys(n_ranks):
    """the SSOR partitions of a launch: key -> number of blocks (equal runs of rows) or None for a caller-given partition"""
    out = {}
    for b in (1, 3, n_ranks, 2 * n_ranks):
        out.setdefault(f"B{b}", b)
    for i in range(len(given_bounds(n_ranks, 100))):
        out[f"given{i}"] = None
    return out


# (kind, steps, degree) of mg_cases.VCYCLE_CONFIGS; SSOR sweeps one block per rank
VCYCLE_CONFIGS = [(k, s, 2 + s % 2) for k in (JACOBI, SSOR, CHEBYSHEV) for s in (1, 2, 3)] + [(SSOR, 0, 2)]


# ------------------------------------------------------------------------------------------------ launches

def group_timeout(group):
    """seconds a rank of this group may take, start-up of the interpreter and the library included.  Measured: two seconds
    for the longest group (a smoother group uploads its hierarchy once per SSOR partition); the library's own waits give up
    after about 15 s and return GMG_ERR_COMM, so nothing that works needs more than this."""
    return 60
