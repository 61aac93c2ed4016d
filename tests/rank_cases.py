"""The operators, vectors and step lists of the rank-parallel tests (DESIGN.md sections 27 and 33).  tests/rank_worker.py runs the
steps of a group on one rank, tests/test_gpu_ranks_reference.py and tests/test_gpu_ranks_layouts.py check what the ranks wrote, tests/test_partition_reference_cpu.py and
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


FIVE_VALUES = np.array([-1 / 6, -1 / 12, 8 / 3, 0.0, 1.25])
SEVEN_MAGNITUDES = np.array([0.25, 0.5, 0.75, 1.0, 0.125, 0.375, 0.625])   # exact in binary: the row sums are exact too


def _csr_of_rows(rows, n_cols):
    rp = np.zeros(len(rows) + 1, dtype=np.int64)
    rp[1:] = np.cumsum([len(c) for c, _ in rows])
    return SimpleNamespace(n_rows=len(rows), n_cols=n_cols, rowptr=rp, col=np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows]),
                           val=np.concatenate([np.asarray(v, dtype=np.float64) for _, v in rows]), nnz=int(rp[-1]))


def _band27(n, rng, distinct, n_classes=0, width=27):
    """banded() of tests/test_gpu_layouts.py: `width` consecutive columns around the diagonal, clipped to [0, n) (the rows at
    the ends are shorter); values from `distinct` or all different; n_classes > 0: full rows take one of that many
    coefficient vectors.  27 consecutive columns are nine runs of three: a 3 x 3 x n lattice in the planner's terms."""
    vectors = [rng.choice(distinct, width) for _ in range(n_classes)] if n_classes else None
    rows = []
    for i in range(n):
        c = sorted({min(n - 1, max(0, i + k - width // 2)) for k in range(width)} | {i})
        if vectors is not None and len(c) == width:
            v = vectors[(i * 7 + i // 64) % n_classes].copy()
        else:
            v = rng.standard_normal(len(c)) if distinct is None else rng.choice(distinct, len(c))
        v[c.index(i)] = 4.0 + abs(v[c.index(i)])
        rows.append((c, v))
    return _csr_of_rows(rows, n)


def _hybrid_spd(n, wide_rows, n_extra=57, shift=0.5):
    """Symmetric, strictly diagonally dominant (SPD): 27 entries per row at row + dz 100 + dy 10 + dx, clipped to [0, n), as the
    operators of tests/test_gpu_hybrid_spmv.py; a wide row couples to n_extra more columns anywhere in [0, n) -- on every
    partition it refers to all the other ranks -- and each of those columns' rows gets the transposed entry (28 entries: its
    slice loses its column pattern and keeps its columns in the stream).  a_ij = -SEVEN_MAGNITUDES[(i + j) % 7] for i != j (a 32nd of that for a wide row's extra entries),
    a_ii = sum_j |a_ij| + shift.  The slices of the wide rows are far beyond the 12 % padding the SELL rule accepts, so the
    operator as a whole is refused and takes the hybrid layout where that is allowed (the system matrix)."""
    rng = np.random.default_rng(28)
    stencil = np.array(sorted(dz * 100 + dy * 10 + dx for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)), dtype=np.int64)
    i = np.arange(n, dtype=np.int64)
    lo, hi = [], []
    for o in stencil[stencil > 0]:
        lo.append(i[: n - o])
        hi.append(i[: n - o] + o)
    for w in wide_rows:
        free = np.setdiff1d(np.setdiff1d(i, w + stencil), np.asarray(wide_rows))
        extra = rng.choice(free, size=n_extra, replace=False)
        lo.append(np.minimum(extra, w))
        hi.append(np.maximum(extra, w))
    n_stencil = sum(len(a) for a in lo[: -len(wide_rows)])
    lo, hi = np.concatenate(lo), np.concatenate(hi)
    assert len(np.unique(lo * n + hi)) == len(lo)
    mag = SEVEN_MAGNITUDES[(lo + hi) % 7]
    mag[n_stencil:] /= 32.0     # (the diagonal of a wide row stays near the others': no outlying eigenvalues for CG to find)
    diag = np.full(n, shift)
    np.add.at(diag, lo, mag)
    np.add.at(diag, hi, mag)
    row = np.concatenate([lo, hi, i])
    col = np.concatenate([hi, lo, i])
    val = np.concatenate([-mag, -mag, diag])
    order = np.lexsort((col, row))
    rp = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rp, row + 1, 1)
    return SimpleNamespace(n_rows=n, n_cols=n, rowptr=np.cumsum(rp), col=col[order].astype(np.int32), val=val[order], nnz=len(row))


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
    if name == "lat21":     # 21 x 17 x 40: on four ranks the two middle chunks are lattice plans, the outer two stay CSR
        return R.lattice_operator(21, 17, 40, None)
    if name == "hybspd":
        return _hybrid_spd(4400, (224, 1500, 2900, 4300))
    if name == "bandfew":
        return _band27(5037, np.random.default_rng(11), FIVE_VALUES, n_classes=7)
    if name == "banddist":
        return _band27(5037, np.random.default_rng(12), None)
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


# ------------------------------------------------------------------------------------------------ device layouts (section 33)

# Operators large enough that a rank's owned rows leave the CSR row-window kernel: what the planner (csrc/gmg_layout.hpp)
# makes of every rank's rows, as stats().spmv0_layout reports it for a level 0 (0 = CSR; else 1 + 2 val8 + 4 col16 + 8
# pattern-run + 16 row classes + 32 lattice window), as the word of the "[gmg]   layout" line of debug_upload for a system
# matrix (only that one may take the hybrid layout), and the lattice window (K plane steps, C columns, rows [R0, R1)).
# tests/layout_roundtrip.cc asserts the same table for its own generators of these operators on the CPU.
LAYOUT_OPERATORS = ("lattice", "lat21", "hybspd", "bandfew", "banddist")
FULL, LATTICE_PLAIN, SELL_FP64, CSR = 63, 1 + 2 + 4 + 32, 1 + 4, 0


def _rank(level0, system, window=None):
    return SimpleNamespace(level0=level0, system=system, window=window)


def _lat37(n_ranks):
    K = {2: 8, 3: 5, 4: 3}[n_ranks]
    R1 = {2: (7196, 7195), 3: (4501, 4501, 4500), 4: (3154, 3154, 3154, 3151)}[n_ranks]
    # the first rank keeps enough whole pattern slices for the pattern-run kernel; a rank with a lower neighbour does not
    return [_rank(FULL if r == 0 or n_ranks == 2 else LATTICE_PLAIN, "sell", (K, 7, 891, R1[r])) for r in range(n_ranks)]


def _bandfew(n_ranks):
    K = {2: 277, 3: 184, 4: 137}[n_ranks]
    R1 = {2: (2506, 2505), 3: (1666, 1666, 1666), 4: (1247, 1247, 1247, 1244)}[n_ranks]
    return [_rank(FULL, "sell", (K, 1, 15, R1[r])) for r in range(n_ranks)]


LAYOUTS = {}
for _n in RANKS:
    LAYOUTS["lattice", _n] = _lat37(_n)
    # thin in x and y: the two outer chunks hold too many boundary rows for SELL and stay CSR (hybrid as a system matrix)
    LAYOUTS["lat21", _n] = [_rank(CSR, "hybrid") for _ in range(_n)]
    LAYOUTS["hybspd", _n] = [_rank(CSR, "hybrid") for _ in range(_n)]
    LAYOUTS["bandfew", _n] = _bandfew(_n)
    LAYOUTS["banddist", _n] = [_rank(SELL_FP64, "sell") for _ in range(_n)]
LAYOUTS["lat21", 4] = [_rank(CSR, "hybrid"), _rank(FULL, "sell", (8, 3, 381, 3191)), _rank(FULL, "sell", (8, 3, 381, 3191)), _rank(CSR, "hybrid")]

# per operator: the option sets its products are taken with.  "upload" options steer the plan and need the operator set
# again; "launch" options are read when the product is launched.
LAYOUT_VARIANTS = {
    "lattice": (("default", {}), ("nolattice", {"disable_lattice": 1}), ("seg1", {"lattice_segments": 1}), ("seg3", {"lattice_segments": 3})),
    "lat21": (("default", {}), ("nolattice", {"disable_lattice": 1}), ("seg1", {"lattice_segments": 1}), ("seg3", {"lattice_segments": 3})),
    "bandfew": (("default", {}), ("nolattice", {"disable_lattice": 1}), ("seg1", {"lattice_segments": 1}), ("seg3", {"lattice_segments": 3})),
    "hybspd": (("default", {}), ("nohybrid", {"disable_hybrid": 1}), ("two", {"hybrid_two_launches": 1})),
    "banddist": (("default", {}),),
}
UPLOAD_OPTIONS = ("disable_lattice", "lattice_segments")


def expected_layout(name, n_ranks, rank, variant):
    """the rank's entry of LAYOUTS under an option set: disable_lattice takes the lattice window away and nothing else"""
    e = LAYOUTS[name, n_ranks][rank]
    if variant == "nolattice":
        return _rank(e.level0 & ~32, e.system, None)
    return e


def layout_spmv_cases():
    return [(name, n) for n in RANKS for name in LAYOUT_OPERATORS]


# coarse CG on a partitioned level 0 that is a lattice plan: 37 x 23 x 19 on 2, 3 and 4 ranks; 21 x 17 x 40 on four, where
# the ranks of one solve run different kernels
LAYOUT_COARSE_KS = {"lattice": (1, 7, 8, 11, 15, 16, 17), "lat21": (1, 7, 8, 9, 15, 16, 17)}


def layout_coarse_operators(n_ranks):
    return ["lattice", "lat21"] if n_ranks == 4 else ["lattice"]


LAYOUT_OUTER = "hybspd"
LAYOUT_OUTER_CASES = [(pc, what) for pc in ("identity", "jacobi") for what in ("zero", "random", "b0", "max_it")]


@functools.lru_cache(maxsize=None)
def x_start(name):
    """a random start vector of the solution's size: b has entries of size 1, so x has entries of the size of 1 / a_ii"""
    m = operator(name)
    return np.random.default_rng(1000 + RHS_SEED[name]).standard_normal(m.n_rows) / np.median(R.diagonal(m))


@functools.lru_cache(maxsize=None)
def outer_case(name, pc, what, tier="seq"):
    """the outer CG cases on an operator of this file: (tol, result); "zero" and "random" stop at cg_reference.OUTER_K,
    "max_it" is refused at cg_reference.OUTER_MAX_IT"""
    m, b, M = operator(name), rhs(name), R.PRECONDS[pc]
    if what == "max_it":
        return R.REFUSE_TOL, R.cg(m, b, R.REFUSE_TOL, R.OUTER_MAX_IT, precond=M, tier=tier)
    x0 = x_start(name) if what == "random" else None
    tol = R.target_tol(R.cg(m, b, 0.0, 40, x0=x0, precond=M, keep_steps=False).history, R.OUTER_K)
    return tol, R.cg(m, b, tol, 1000, x0=x0, precond=M, tier=tier)


def layout_solve_results(tier):
    """x of every solve of the layout groups that cg_reference.gpu_cases() does not hold, in one tier"""
    out = [stop_case(name, k, tier)[1].x for name in LAYOUT_COARSE_KS for k in LAYOUT_COARSE_KS[name] if name in RHS_SEED]
    return out + [outer_case(LAYOUT_OUTER, pc, what, tier)[1].x for pc, what in LAYOUT_OUTER_CASES if what != "b0"]


@functools.lru_cache(maxsize=None)
def layout_spread():
    """S of cg_reference.spread() over the solves of layout_solve_results() alone"""
    xs = [layout_solve_results(t) for t in R.TIERS]
    s = 0.0
    for i in range(len(xs[0])):
        scale = np.abs(xs[0][i]).max()
        for a in range(3):
            for b in range(a + 1, 3):
                s = max(s, float(np.abs(xs[a][i] - xs[b][i]).max() / scale))
    return s


# ------------------------------------------------------------------------------------------------ coarse CG

COARSE_OPERATORS = ("csr", "band9", "tri257", "blocks", "wide")  # "blocks" on two ranks only
COARSE_KS = {"csr": (1, 7, 8, 9, 15, 16, 17), "band9": (1, 7, 8, 9, 15, 16, 17), "tri257": (1, 7, 8, 9, 15, 16, 17),
             "blocks": (1, 7, 8, 9, 15, 16, 17), "wide": (1, 7, 8, 9, 15, 16, 17)}
COARSE_CHUNKS = (0, 1, 3)
RHS_SEED = {"wide": 8, "blocks": 9, "lat21": 11, "hybspd": 12}   # (lat21: seed 10 leaves 7 and 9 not targetable)


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
    ks = dict(COARSE_KS, **LAYOUT_COARSE_KS)
    return [(name, k) for name in ks for k in ks[name] if (name, k) not in have]


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
