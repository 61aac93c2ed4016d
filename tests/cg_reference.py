"""A plain restatement of deal.II's SolverCG with a SolverControl-style check, and the SPD operators, cases and tolerances of
tests/test_gpu_coarse_cg.py.  Written from the definition of the method; it shares no code with csrc/ or oracle/.

    x = x0 (or 0);  g = A x - b (or -b);  res = |g|;  stop if res <= tol (success) or max_it == 0 / res is NaN (failure)
    d = -M g;  gh = g . M g
    iteration it = 1, 2, ...:
        h = A d;  alpha = gh / (d . h);  x += alpha d;  g += alpha h;  res = |g|
        success if res <= tol;  failure if it >= max_it or res is NaN  (the iterate stays in x either way)
        gh_new = g . M g;  beta = gh_new / gh;  d = beta d - M g

Three tiers differ in how sums are formed and in the number format:
    "seq"   fp64, dot products added element after element (numpy.cumsum)
    "pair"  fp64, numpy's pairwise sums
    "ld"    numpy.longdouble throughout (operator, vectors, sums); results rounded to fp64 at the end
A matrix row is summed in stored order in every tier (a padded table, one column of it after the other).

The device's reductions (workgroup partials added by strided threads) are one more summation order of the kind that separates
"seq" from "pair", so the tolerance on x is taken from the spread S of the tiers over all GPU cases: X_TOL_FACTOR * S,
relative to max|x| (spread(), x_tolerance(); the two cases of 200 000 rows have an S of their own).  Nothing here looks at what the device returns."""
import functools
import itertools
from types import SimpleNamespace

import numpy as np

OK, NOCONV = 0, 1
TIERS = ("seq", "pair", "ld")
X_TOL_FACTOR = 64.0
MARGIN = 1.05          # target_tol: res_k <= tol / MARGIN and res_j >= MARGIN tol for j < k
SENSITIVITY = 100.0    # every step alpha_j d_j of a GPU case is larger than this many tolerances


# ---------------------------------------------------------------------------------------------- arithmetic of one tier

class _Tier:
    def __init__(self, name):
        self.name = name
        self.dtype = np.longdouble if name == "ld" else np.float64

    def vec(self, a):
        return np.array(a, dtype=self.dtype)

    def dot(self, a, b):
        p = a * b
        if p.size == 0:
            return self.dtype(0.0)
        return np.cumsum(p)[-1] if self.name == "seq" else np.sum(p)


def _table(m, dtype):
    """(col, val, width): the rows padded to the widest one with (column 0, +0.0) behind their stored entries"""
    rp = np.asarray(m.rowptr, dtype=np.int64)
    n = int(m.n_rows)
    length = rp[1:] - rp[:-1]
    w = int(length.max()) if n else 0
    k = np.arange(w)
    ok = k[None, :] < length[:, None]
    at = np.minimum(rp[:-1, None] + k[None, :], max(len(m.col) - 1, 0))
    col = np.where(ok, np.asarray(m.col, dtype=np.int64)[at], 0) if w else np.zeros((n, 0), dtype=np.int64)
    val = np.where(ok, np.asarray(m.val, dtype=np.float64)[at], 0.0).astype(dtype) if w else np.zeros((n, 0), dtype=dtype)
    return col, val, ok


def matvec(table, x):
    """y_i = sum over the stored entries of row i, in stored order (padding entries are skipped, not added as zeros)"""
    col, val, ok = table
    y = np.zeros(col.shape[0], dtype=x.dtype)
    for j in range(col.shape[1]):
        y = np.where(ok[:, j], y + val[:, j] * x[col[:, j]], y)
    return y


def diagonal(m):
    rp = np.asarray(m.rowptr, dtype=np.int64)
    row = np.repeat(np.arange(m.n_rows), rp[1:] - rp[:-1])
    on = np.asarray(m.col) == row
    d = np.zeros(m.n_rows)
    d[row[on]] = np.asarray(m.val)[on]
    return d


def identity(m, tier):
    return None


def jacobi(m, tier, omega=0.6):
    """M = omega D^-1 (PreconditionJacobi): M g = (omega g) * (1 / a_ii)"""
    invd = _Tier(tier).vec(1.0) / _Tier(tier).vec(diagonal(m))
    om = _Tier(tier).dtype(omega)
    return lambda g: (om * g) * invd


# ---------------------------------------------------------------------------------------------- the solver

def cg(m, b, tol, max_it, x0=None, precond=identity, tier="seq", keep_steps=True):
    """SolverCG on the CSR namespace m.  Returns x (fp64), iterations, status (OK / NOCONV), history (res_0 ... res_it as
    fp64) and steps (alpha_j d_j as fp64, j = 0 ... it - 1)."""
    T = _Tier(tier)
    A = _table(m, T.dtype)
    M = precond(m, tier)
    b = T.vec(b)
    tol = T.dtype(tol)
    if x0 is None or not np.any(np.asarray(x0)):
        x = T.vec(np.zeros(m.n_rows))
        g = -b
    else:
        x = T.vec(x0)
        g = matvec(A, x) - b
    res = np.sqrt(T.dot(g, g))
    history, steps = [float(res)], []
    it, status = 0, None

    def check():
        if res <= tol:
            return OK
        if it >= max_it or np.isnan(res):
            return NOCONV
        return None

    status = check()
    if status is None:
        if M is None:
            d, gh = -g, res * res
        else:
            h = M(g)
            d, gh = -h, T.dot(g, h)
    while status is None:
        it += 1
        h = matvec(A, d)
        alpha = gh / T.dot(d, h)
        step = alpha * d
        x = x + step
        g = g + alpha * h
        res = np.sqrt(T.dot(g, g))
        history.append(float(res))
        if keep_steps:
            steps.append(np.asarray(step, dtype=np.float64))
        status = check()
        if status is not None:
            break
        if M is None:
            gh_new = res * res
            beta = gh_new / gh
            d = beta * d - g
        else:
            h = M(g)
            gh_new = T.dot(g, h)
            beta = gh_new / gh
            d = beta * d - h
        gh = gh_new
    return SimpleNamespace(x=np.asarray(x, dtype=np.float64), iterations=it, status=status, history=np.array(history), steps=steps,
                           res=history[-1])


def target_tol(history, k, floor=0.0):
    """A tolerance at which the solve with this residual history stops at exactly iteration k: the geometric mean of res_k and
    the smallest earlier residual.  Raises unless res_k <= tol / MARGIN and res_j >= MARGIN tol for every j < k (a condition
    on the inputs: when it fails, the case takes another rhs seed).  `floor` stands in for a res_k below it: a solve that is
    exact after k steps (n = 1) leaves a residual of 0 here and of a few roundings of res_0 elsewhere."""
    history = np.asarray(history, dtype=np.float64)
    if not 1 <= k < len(history):
        raise ValueError(f"iteration {k} is outside the history (0 ... {len(history) - 1})")
    before = history[:k].min()
    tol = float(np.sqrt(max(history[k], floor) * before))
    if not (history[k] <= tol / MARGIN and before >= MARGIN * tol) or not np.isfinite(tol) or tol <= 0.0:
        raise ValueError(f"iteration {k} is not targetable: res_k {history[k]:.3e}, smallest earlier residual {before:.3e}")
    return tol


# ---------------------------------------------------------------------------------------------- SPD operators

def _csr_from_table(n, ok, col, val):
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(ok.sum(axis=1))
    return SimpleNamespace(n_rows=n, n_cols=n, rowptr=rp, col=col[ok].astype(np.int32), val=val[ok].astype(np.float64), nnz=int(rp[-1]))


def tridiagonal_operator(n):
    """symmetric tridiagonal, off-diagonals -1, diagonal 2.5 + 0.4 sin(0.7 i) (strictly dominant: eigenvalues in [0.1, 4.9])"""
    i = np.arange(n, dtype=np.int64)
    ok = np.stack([i > 0, np.ones(n, bool), i < n - 1], axis=1)
    col = np.stack([np.maximum(i - 1, 0), i, np.minimum(i + 1, n - 1)], axis=1)
    val = np.stack([np.full(n, -1.0), 2.5 + 0.4 * np.sin(0.7 * i), np.full(n, -1.0)], axis=1)
    return _csr_from_table(n, ok, col, val)


def banded_operator(n, per_side, seed, period=4, reach=60, shift=0.25):
    """Symmetric, strictly diagonally dominant, 2 per_side + 1 entries per row away from the ends.  Row i couples to i + o for
    the per_side offsets o of its residue class i mod period; all offsets are multiples of the period, so i - o is of the same
    class and the pattern is symmetric.  The classes use disjoint offsets: a slice of 64 rows sees period * 2 * per_side + 1
    different column distances and no row pattern repeats.  Values: a_(i, i+o) = -u(i, o), u uniform in (0.25, 1);
    a_ii = sum |off-diagonals| + shift (1 + u_i)."""
    rng = np.random.default_rng(seed)
    assert period * per_side <= reach
    pool = rng.permutation(np.arange(1, reach + 1))[: period * per_side].reshape(period, per_side) * period
    offs = np.sort(pool, axis=1)                                   # [class, per_side], ascending
    i = np.arange(n, dtype=np.int64)
    fwd_col = i[:, None] + offs[i % period]                        # [n, per_side]
    fwd_ok = fwd_col < n
    fwd_val = -(0.25 + 0.75 * rng.random((n, per_side)))
    bwd_col = i[:, None] - offs[i % period][:, ::-1]               # ascending columns
    bwd_ok = bwd_col >= 0
    # a_(i, i-o) = a_(i-o, i): the forward value of row i - o at the same offset
    src_row = np.where(bwd_ok, bwd_col, 0)
    bwd_val = fwd_val[src_row, np.arange(per_side)[::-1][None, :]]
    off_sum = np.where(fwd_ok, -fwd_val, 0.0).sum(axis=1) + np.where(bwd_ok, -bwd_val, 0.0).sum(axis=1)
    diag = off_sum + shift * (1.0 + rng.random(n))
    ok = np.concatenate([bwd_ok, np.ones((n, 1), bool), fwd_ok], axis=1)
    col = np.concatenate([src_row, i[:, None], np.where(fwd_ok, fwd_col, 0)], axis=1)
    val = np.concatenate([bwd_val, diag[:, None], fwd_val], axis=1)
    return _csr_from_table(n, ok, col, val)


def lattice_operator(nx, ny, nz, rng, dirichlet=True):
    """27-point operator on an nx x ny x nz lattice, lexicographic numbering (x fastest), CSR with ascending columns.
    Boundary vertices are Dirichlet rows (diagonal by vertex type, stored zeros towards their existing neighbours);
    interior rows have zeros in the columns of boundary vertices (the eliminated couplings the reference keeps as stored
    zeros); the interior coefficients are the Q1 Laplace stencil's values times h."""
    h = 0.25
    w = np.empty((3, 3, 3))
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                m = abs(dz - 1) + abs(dy - 1) + abs(dx - 1)
                w[dz, dy, dx] = h * (8.0 / 3.0, 0.0, -1.0 / 6.0, -1.0 / 12.0)[m]
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.int32), np.arange(ny, dtype=np.int32), np.arange(nx, dtype=np.int32), indexing="ij")
    x, y, z = x.ravel(), y.ravel(), z.ravel()
    n = nx * ny * nz
    bnd = ((x == 0) | (x == nx - 1) | (y == 0) | (y == ny - 1) | (z == 0) | (z == nz - 1)) if dirichlet else np.zeros(n, bool)
    kind = (x == 0).astype(np.int8) + (x == nx - 1) + (y == 0) + (y == ny - 1) + (z == 0) + (z == nz - 1)
    # (n, 27) tables in offset order = ascending column order inside a row: no sort needed
    ok = np.empty((n, 27), dtype=bool)
    col = np.empty((n, 27), dtype=np.int32)
    val = np.empty((n, 27), dtype=np.float64)
    row = np.arange(n, dtype=np.int64)
    j = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                o = (x + dx >= 0) & (x + dx < nx) & (y + dy >= 0) & (y + dy < ny) & (z + dz >= 0) & (z + dz < nz)
                c = row + (dx + nx * dy + nx * ny * dz)
                cc = np.where(o, c, 0)
                v = np.where(bnd | bnd[cc], 0.0, w[dz + 1, dy + 1, dx + 1])  # eliminated rows / columns: stored zeros
                if dz == dy == dx == 0:
                    v = np.where(bnd, h * (4.0 / 3.0) / np.maximum(kind, 1), w[1, 1, 1])
                ok[:, j], col[:, j], val[:, j] = o, cc, v
                j += 1
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(ok.sum(axis=1))
    return SimpleNamespace(n_rows=n, n_cols=n, rowptr=rp, col=col[ok], val=val[ok], nnz=int(rp[-1]))


def q1_cell_matrix(h, rng):
    """Q1 Laplace cell matrix on a cube of edge h (the reference's K_e) with a small random diagonal
    that breaks the symmetry between the vertices of a cell: the sums must follow the cell order"""
    Ke = np.zeros((8, 8))
    for a in range(8):
        for b in range(8):
            m = bin(a ^ b).count("1")
            Ke[a, b] = h * (1.0 / 3.0, 0.0, -1.0 / 12.0, -1.0 / 12.0)[m]
    Ke += 1e-3 * np.diag(rng.random(8))
    return Ke


def cell_matrix_operator(shape, Ke):
    """host-style assembly on an nx x ny x nz vertex lattice: cells in lexicographic order, every cell adds Ke; boundary rows
    keep sum |Ke[a][a]|; CSR pattern = all pairs sharing a cell"""
    nx, ny, nz = shape
    n = nx * ny * nz
    bnd = np.zeros((nz, ny, nx), bool)
    bnd[0], bnd[-1], bnd[:, 0], bnd[:, -1], bnd[:, :, 0], bnd[:, :, -1] = True, True, True, True, True, True
    bnd = bnd.ravel()
    dense = {}
    for cz, cy, cx in itertools.product(range(nz - 1), range(ny - 1), range(nx - 1)):
        d = [cx + (a & 1) + nx * (cy + ((a >> 1) & 1)) + nx * ny * (cz + ((a >> 2) & 1)) for a in range(8)]
        for a in range(8):
            for b in range(8):
                key = (d[a], d[b])
                dense.setdefault(key, 0.0)
            if bnd[d[a]]:
                dense[(d[a], d[a])] += abs(Ke[a, a])
            else:
                for b in range(8):
                    if not bnd[d[b]]:
                        dense[(d[a], d[b])] += Ke[a, b]
    keys = sorted(dense)
    rows = np.array([k[0] for k in keys]); cols = np.array([k[1] for k in keys], dtype=np.int32)
    rp = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rp, rows + 1, 1)
    return SimpleNamespace(n_rows=n, n_cols=n, rowptr=np.cumsum(rp), col=cols, val=np.array([dense[k] for k in keys]), nnz=len(keys))


# ---------------------------------------------------------------------------------------------- the GPU cases

STOP_KS = (1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25)
LATTICE_KS = (1, 2, 7, 8, 11, 15, 16, 17, 23, 24, 25)       # 37 x 23 x 19: 9 is not targetable there, 11 replaces it
FORMED_SHAPE = (9, 7, 6)
FORMED_KS = (1, 2, 7, 8, 9, 15, 16, 17, 23, 25)             # 24 is not targetable there; the solve takes 31 at 1e-10
SEQUENCE = (("stop", 25), ("stop", 3), ("stop", 20), ("zero", 0), ("stop", 9), ("refuse", 5), ("stop", 17))
REFUSE_MAX_ITS = (1, 5, 7, 8, 9, 16)
REFUSE_TOL = 1e-200
LENGTHS = (1, 2, 3, 255, 256, 257, 511, 512, 513)
LENGTH_K = {1: 1, 2: 2, 3: 3}                               # longer ones stop at iteration 9: one past the ring
VARIANT_SIZES = (199999, 200000)
VARIANT_K = 5
COMM_KS = (7, 8, 9)
OUTER_K = 16
OUTER_MAX_IT = 9
PRECONDS = {"identity": identity, "jacobi": jacobi}


@functools.lru_cache(maxsize=None)
def operator(name):
    """The operators of the GPU cases by name -> (CSR namespace, seed of the rhs)."""
    if name == "csr":          # thin lattice: mostly boundary rows, stays on the CSR row-window kernel
        return lattice_operator(13, 11, 9, None), 1
    if name == "sell":         # 27 per row, no repeating pattern: plain SELL-64 with 16-bit column offsets
        return banded_operator(64 * 40 + 17, 13, seed=5, shift=1.0), 2
    if name == "band9":        # 9 per row: padding to 12 is beyond what SELL-64 accepts, stays CSR
        return banded_operator(1500, 4, seed=6, period=2, reach=20), 3
    if name == "lattice":
        return lattice_operator(37, 23, 19, None), 4
    if name == "formed":
        return cell_matrix_operator(FORMED_SHAPE, formed_cell_matrix()), 5
    if name == "small":        # outer CG on few rows next to the 13 x 11 x 9 system
        return lattice_operator(6, 5, 5, None), 6
    if name.startswith("tri"):
        return tridiagonal_operator(int(name[3:])), 7
    raise KeyError(name)


def formed_cell_matrix():
    return q1_cell_matrix(0.25, np.random.default_rng(97))


@functools.lru_cache(maxsize=None)
def rhs(name):
    m, seed = operator(name)
    return np.random.default_rng(seed).standard_normal(m.n_rows)


@functools.lru_cache(maxsize=None)
def x_start(name):
    m, seed = operator(name)
    return np.random.default_rng(1000 + seed).standard_normal(m.n_rows)


@functools.lru_cache(maxsize=None)
def full_history(name, precond="identity", start="zero", n_it=40, tier="seq"):
    """residuals of n_it iterations without a stopping tolerance"""
    m, _ = operator(name)
    x0 = x_start(name) if start == "random" else None
    return cg(m, rhs(name), 0.0, n_it, x0=x0, precond=PRECONDS[precond], tier=tier, keep_steps=False).history


@functools.lru_cache(maxsize=None)
def stop_case(name, k, precond="identity", start="zero", tier="seq"):
    """the solve on operator `name` that stops at iteration k: (tol, result of cg)"""
    m, _ = operator(name)
    hist = full_history(name, precond, start)
    # (one row: CG is exact after its only step, the residual left is rounding, 2^-53 res_0 stands in for it)
    tol = target_tol(hist, k, floor=2.0 ** -53 * hist[0] if m.n_rows == 1 else 0.0)
    x0 = x_start(name) if start == "random" else None
    return tol, cg(m, rhs(name), tol, 1000, x0=x0, precond=PRECONDS[precond], tier=tier)


@functools.lru_cache(maxsize=None)
def refused_case(name, max_it, precond="identity", tier="seq"):
    m, _ = operator(name)
    return REFUSE_TOL, cg(m, rhs(name), REFUSE_TOL, max_it, precond=PRECONDS[precond], tier=tier)


@functools.lru_cache(maxsize=None)
def converged_start_case(precond="identity", tier="seq"):
    """outer CG entered with a start vector that already meets the tolerance: x0 is the solution of the solve that stops at
    iteration 25, the tolerance that of the solve that stops at OUTER_K -> (x0, tol, result with 0 iterations)"""
    m, _ = operator("csr")
    x0 = stop_case("csr", 25, precond)[1].x
    tol = stop_case("csr", OUTER_K, precond)[0]
    return x0, tol, cg(m, rhs("csr"), tol, 1000, x0=x0, precond=PRECONDS[precond], tier=tier)


def length_k(n):
    return LENGTH_K.get(n, 9)


def gpu_cases():
    """every (kind, operator, k or max_it, preconditioner, start) the GPU file solves with a nonzero number of iterations"""
    out = []
    for name in ("csr", "sell"):
        out += [("stop", name, k, "identity", "zero") for k in STOP_KS]
    out += [("stop", "lattice", k, "identity", "zero") for k in LATTICE_KS]
    out += [("stop", "formed", k, "identity", "zero") for k in FORMED_KS]
    out += [("stop", "band9", k, "identity", "zero") for k in (8, 9)]
    out += [("stop", "csr", k, "identity", "zero") for kind, k in SEQUENCE if kind == "stop"]
    for name in ("csr", "sell"):
        out += [("refuse", name, mi, "identity", "zero") for mi in REFUSE_MAX_ITS]
    out += [("stop", f"tri{n}", length_k(n), "identity", "zero") for n in LENGTHS]
    out += [("stop", f"tri{n}", VARIANT_K, "identity", "zero") for n in VARIANT_SIZES]
    for pc in PRECONDS:
        out += [("stop", "csr", OUTER_K, pc, "zero"), ("stop", "csr", OUTER_K, pc, "random"), ("refuse", "csr", OUTER_MAX_IT, pc, "zero")]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


def case_result(case, tier="seq"):
    kind, name, k, pc, start = case
    if kind == "stop":
        return stop_case(name, k, pc, start, tier)[1]
    return refused_case(name, k, pc, tier)[1]


LARGE_ROWS = 100000


def is_large(name):
    return operator(name)[0].n_rows >= LARGE_ROWS


@functools.lru_cache(maxsize=None)
def spread(large=False):
    """S: the largest deviation of x between the three tiers over all GPU cases, relative to max|x|.  The two cases of
    200 000 rows (the switch between the variants) have an S of their own: the rounding of a sequential dot product grows
    with its length, and their S, four times that of all others, would widen every other case's tolerance."""
    s = 0.0
    for case in gpu_cases():
        if is_large(case[1]) != large:
            continue
        xs = [case_result(case, t).x for t in TIERS]
        scale = np.abs(xs[0]).max()
        for a, b in itertools.combinations(xs, 2):
            s = max(s, float(np.abs(a - b).max() / scale))
    return s


def x_tolerance(name="csr"):
    """tolerance on the device's x for a case on operator `name`, relative to max|x| of the reference"""
    return X_TOL_FACTOR * spread(is_large(name))
