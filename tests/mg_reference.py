"""The smoothers and the V-cycle of the multigrid preconditioner, written from their definitions (DESIGN.md
section 16).  Nothing here is taken from oracle/gmg_oracle.c or from csrc/: the smoothers are closed-form operators, not the
sweeps and the three-term recurrence the oracle and the device run.

    Jacobi      S = omega D^-1
    SSOR        S = blockdiag_b [ omega (2 - omega) (D_b + omega U_b)^-1 D_b (D_b + omega L_b)^-1 ],  A_bb = L_b + D_b + U_b the
                diagonal block of rows [n b // B, n (b + 1) // B) with its off-block columns dropped, B clipped to ceil(n / 64),
                or the caller's bounds; the two factors are inverted by triangular solves
    Chebyshev   S = q(D^-1 A) D^-1,  1 - x q(x) = T_k((beta + alpha - 2 x) / (beta - alpha)) / T_k((beta + alpha) / (beta - alpha)),
                beta = lmax, alpha = lmax / ratio, lmax = max_i sum_j |a_ij| / |a_ii| or the user's value
    apply       s steps of u <- u + S (rhs - A u) from u = 0;  smooth: the same from the given u;  s = 0 leaves u as it is
                (apply: the caller's u, not 0 -- include/gmg_coulomb.h)
    V-cycle     level 0: u = A_0^-1 d exactly;  level l > 0: u = apply(d); t = d - (A_l + I_l) u; d_{l-1} += P_{l-1}^T t; recurse;
                u += P_{l-1} u_{l-1}; d -= I_l^T u; u = smooth(u, d)
    M           dst = 0; d_l[copy_level_l] = src[copy_global_l] on zeroed d_l; V-cycle; dst[copy_global_l] = u_l[copy_level_l]

Two tiers (TIERS): "f64" (scipy.sparse products, SuperLU triangular solves and level-0 factorisation, q as a polynomial from
numpy.polynomial evaluated by Horner's rule on D^-1 A) and "ld" (numpy.longdouble throughout: products row by row, triangular solves
by substitution, A_0^-1 by refinement of the factorisation with longdouble residuals until it stalls, q through the roots of T_k:
1 - x q(x) = prod_j (1 - x / x_j)).  A third evaluation of q, through the eigen-decomposition of D^-1/2 A D^-1/2, is
chebyshev_by_eig (the CPU tests compare all three).  The spread of the tiers on a case is its rounding scale S_case; the
tolerance on a device vector is TOL_FACTOR S_case ||ref||_2 + the coarse allowance, in the 2-norm (tolerance()).

The coarse allowance: the result is affine in the level-0 solution, result = M src + T (u_0 - A_0^-1 d_0), T = coarse_map().
A CG stopped at ||d_0 - A_0 u_0||_2 <= tau leaves ||u_0 - A_0^-1 d_0||_2 <= tau / lambda_min(A_0); the direct solver leaves at
most c u kappa_2 ||A_0^-1 d_0||_2 (tests/fastdiag_reference.py).  Each times ||T||_2.

MUTATIONS are the wrong derivations the tests must be able to see; every one is a flag of the reference itself."""
import functools
from dataclasses import dataclass, field, replace

import numpy as np

JACOBI, SSOR, CHEBYSHEV = 0, 1, 2
KIND_NAMES = {JACOBI: "jacobi", SSOR: "ssor", CHEBYSHEV: "chebyshev"}
TIERS = ("f64", "ld")
U = 2.0 ** -53
TOL_FACTOR = 64.0        # a different but equally valid summation order
SENSITIVITY = 1000.0     # every kept (case, mutation) pair differs by this many tolerances

MUTATIONS = (
    "drop_edge_out",          # t = d - A u, without I u
    "drop_edge_in",           # no d -= I^T u
    "edge_in_before_prolong", # d -= I^T u with u before u += P u_c
    "one_step_fewer",         # s - 1 steps
    "apply_not_from_zero",    # apply starts from the caller's u
    "ssor_omega_factor",      # omega (2 - omega) -> omega
    "cheb_interval",          # the ratio on the wrong side: [lmax, lmax ratio].  (alpha and beta merely exchanged is the SAME
                              # polynomial, T_k being even or odd: test_chebyshev_exchange_is_identity)
    "ssor_coupled",           # the blocks not decoupled: one block
    "no_zero_dst",            # copy_from_mg without dst = 0
    "skip_copy_entry",        # the last copy-list entry of the finest level left out, both ways
)


@dataclass(frozen=True)
class Config:
    kind: int = SSOR
    omega: float = 0.5
    steps: int = 2
    degree: int = 2
    ratio: float = 30.0
    lmax: float = 0.0            # > 0: the user's bound
    blocks: int = 1
    bounds: tuple = ()           # ((level, (b_0, ..., b_B)), ...): caller-given SSOR partitions
    mut: frozenset = field(default_factory=frozenset)

    def with_mut(self, *names):
        assert all(n in MUTATIONS for n in names)
        return replace(self, mut=frozenset(names))

    def label(self):
        s = f"{KIND_NAMES[self.kind]}-s{self.steps}"
        if self.kind == CHEBYSHEV:
            s += f"-k{self.degree}-r{self.ratio:g}" + (f"-l{self.lmax:g}" if self.lmax > 0 else "")
        if self.kind == SSOR:
            s += f"-B{self.blocks}" + ("-given" if self.bounds else "")
        return s


# ------------------------------------------------------------------------------------------------ operators of one tier

def _scipy_csr(m):
    import scipy.sparse as sp

    a = sp.csr_matrix((np.asarray(m.val, dtype=np.float64), np.asarray(m.col, dtype=np.int64), np.asarray(m.rowptr, dtype=np.int64)),
                      shape=(int(m.n_rows), int(m.n_cols)))
    a.sum_duplicates()
    a.sort_indices()
    return a


class _Op:
    """a sparse operator in one tier: mv (A X), tmv (A^T X) on arrays [n, k]"""

    def __init__(self, a, dtype):
        self.sp, self.dtype = a, dtype
        self.shape = a.shape
        if dtype is not np.float64:
            self._t = a.T.tocsr()
            self._t.sort_indices()

    def _rows(self, a, x):
        out = np.zeros((a.shape[0], x.shape[1]), dtype=self.dtype)
        if a.nnz == 0:
            return out
        prod = a.data.astype(self.dtype)[:, None] * x[a.indices]
        start = a.indptr[:-1]
        full = a.indptr[1:] > start
        out[full] = np.add.reduceat(prod, start[full], axis=0)
        return out

    def mv(self, x):
        return self.sp @ x if self.dtype is np.float64 else self._rows(self.sp, x)

    def tmv(self, x):
        return self.sp.T @ x if self.dtype is np.float64 else self._rows(self._t, x)


def _tri_solve_ld(t, omega, b, lower):
    """(D + omega T_off)^-1 b by substitution in longdouble; t: scipy CSR holding the diagonal and one strict triangle"""
    n = t.shape[0]
    x = np.zeros_like(b)
    ptr, idx, val = t.indptr, t.indices, t.data.astype(np.longdouble)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        c, v = idx[ptr[i]:ptr[i + 1]], val[ptr[i]:ptr[i + 1]]
        off = c != i
        acc = b[i] - omega * (v[off, None] * x[c[off]]).sum(axis=0) if off.any() else b[i]
        x[i] = acc / v[~off][0]
    return x


class Level:
    """one level of one hierarchy in one tier"""

    def __init__(self, A, I, P_down, dtype):
        self.dtype = dtype
        self.A = _Op(A, dtype)
        self.I = _Op(I, dtype) if I is not None and I.nnz > 0 else None
        self.P = _Op(P_down, dtype) if P_down is not None else None   # level - 1 -> level
        self.n = A.shape[0]
        self.diag = A.diagonal().astype(dtype)
        self.gershgorin = float((abs(A).sum(axis=1).A1 / np.abs(A.diagonal())).max())
        self._blocks = {}

    # ---- S R for the three smoothers ----------------------------------------------------------------------------
    def block_bounds(self, cfg, level):
        for lv, b in cfg.bounds:
            if lv == level:
                return [int(v) for v in b]
        if "ssor_coupled" in cfg.mut:
            return [0, self.n]
        B = max(1, min(int(cfg.blocks), (self.n + 63) // 64))
        return [self.n * b // B for b in range(B + 1)]

    def _block(self, rb, re):
        import scipy.sparse as sp

        if (rb, re) not in self._blocks:
            a = self.A.sp[rb:re, rb:re].tocsr()
            lo, up = sp.tril(a, 0, format="csr"), sp.triu(a, 0, format="csr")
            for t in (lo, up):
                t.sort_indices()
            self._blocks[(rb, re)] = (lo, up, a.diagonal())
        return self._blocks[(rb, re)]

    def ssor(self, cfg, level, r):
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla

        om = self.dtype(cfg.omega)
        factor = om if "ssor_omega_factor" in cfg.mut else om * (2 - om)
        y = np.zeros_like(r)
        bounds = self.block_bounds(cfg, level)
        assert bounds[0] == 0 and bounds[-1] == self.n and all(a <= b for a, b in zip(bounds, bounds[1:]))
        for rb, re in zip(bounds, bounds[1:]):
            if re == rb:
                continue
            lo, up, d = self._block(rb, re)
            if self.dtype is np.float64:
                D = sp.diags(d)
                fl = (D + cfg.omega * sp.tril(lo, -1)).tocsr()
                fu = (D + cfg.omega * sp.triu(up, 1)).tocsr()
                z = spla.spsolve_triangular(fl, r[rb:re], lower=True)
                y[rb:re] = factor * spla.spsolve_triangular(fu, d[:, None] * z, lower=False)
            else:
                z = _tri_solve_ld(lo, om, r[rb:re], True)
                y[rb:re] = factor * _tri_solve_ld(up, om, d.astype(self.dtype)[:, None] * z, False)
        return y

    def cheb_interval(self, cfg):
        lmax = cfg.lmax if cfg.lmax > 0 else self.gershgorin
        if "cheb_interval" in cfg.mut:
            return lmax, lmax * cfg.ratio
        return lmax / cfg.ratio, lmax

    def chebyshev(self, cfg, r):
        alpha, beta = self.cheb_interval(cfg)
        k = int(cfg.degree)
        z = r / self.diag[:, None]
        if self.dtype is np.float64:
            from numpy.polynomial import Chebyshev, Polynomial

            c = Chebyshev.basis(k, domain=[alpha, beta]).convert(kind=Polynomial, domain=[-1, 1], window=[-1, 1])
            p = c / c(0.0)                       # 1 - x q(x)
            q, rem = divmod(Polynomial([1.0]) - p, Polynomial([0.0, 1.0]))
            assert abs(rem.coef).max() <= 64 * U
            y = q.coef[-1] * z
            for a in q.coef[-2::-1]:             # Horner on B = D^-1 A:  y <- a z + B y
                y = a * z + self.A.mv(y) / self.diag[:, None]
            return y
        ld = np.longdouble
        pi = ld("3.14159265358979323846264338327950288")
        j = np.arange(1, k + 1).astype(ld)
        roots = (ld(beta) + ld(alpha) - (ld(beta) - ld(alpha)) * np.cos(pi * (2 * j - 1) / (2 * k))) / 2
        y = np.zeros_like(r)                     # (I - prod_j (I - B / x_j)) B^-1 z, factor by factor
        for x in roots:
            y = y + (z - self.A.mv(y) / self.diag[:, None]) / x
        return y

    def S(self, cfg, level, r):
        if cfg.kind == JACOBI:
            return self.dtype(cfg.omega) * r / self.diag[:, None]
        if cfg.kind == SSOR:
            return self.ssor(cfg, level, r)
        return self.chebyshev(cfg, r)

    def steps(self, cfg, level, u, rhs, from_zero):
        s = int(cfg.steps) - (1 if "one_step_fewer" in cfg.mut else 0)
        if s <= 0:
            return u
        if from_zero and "apply_not_from_zero" not in cfg.mut:
            u = np.zeros_like(rhs)
        for _ in range(s):
            u = u + self.S(cfg, level, rhs - self.A.mv(u))
        return u


def chebyshev_by_eig(A, cfg, r):
    """q(D^-1 A) D^-1 r through the eigen-decomposition of D^-1/2 A D^-1/2 (fp64, dense): the third evaluation"""
    from numpy.polynomial import chebyshev as C

    a = A.toarray()
    d = np.diag(a).copy()
    assert np.abs(a - a.T).max() <= 8 * U * np.abs(a).max()
    lam, V = np.linalg.eigh((a + a.T) / 2 / np.sqrt(d)[:, None] / np.sqrt(d)[None, :])
    lmax = cfg.lmax if cfg.lmax > 0 else float((np.abs(a).sum(axis=1) / np.abs(d)).max())
    alpha, beta = lmax / cfg.ratio, lmax
    e = np.zeros(cfg.degree + 1)
    e[-1] = 1.0
    p = C.chebval((beta + alpha - 2 * lam) / (beta - alpha), e) / C.chebval((beta + alpha) / (beta - alpha), e)
    q = (1 - p) / lam
    return (V @ (q[:, None] * (V.T @ (r / np.sqrt(d)[:, None])))) / np.sqrt(d)[:, None]


# ------------------------------------------------------------------------------------------------ a hierarchy

class Hierarchy:
    """what the reference reads of a hierarchy (level_matrices, edge_matrices, prolongations, copy_global, copy_level,
    system_matrix), per tier"""

    def __init__(self, hier, name="?"):
        self.name = name
        self.raw = hier
        self.n_levels = len(hier.level_matrices)
        self.n_sys = int(hier.system_matrix.n_rows)
        self.copy_global = [np.asarray(g, dtype=np.int64) for g in hier.copy_global]
        self.copy_level = [np.asarray(v, dtype=np.int64) for v in hier.copy_level]
        for g, v in zip(self.copy_global, self.copy_level):
            assert len(set(g.tolist())) == len(g) and len(set(v.tolist())) == len(v)
        A = [_scipy_csr(m) for m in hier.level_matrices]
        I = [None if m is None or m.nnz == 0 else _scipy_csr(m) for m in hier.edge_matrices]
        P = [None] + [_scipy_csr(m) for m in hier.prolongations]
        self._csr = (A, I, P)
        self.A, self.I, self.P = A, I, P   # scipy CSR per level: A_l, I_l (None without edges), P_l: level l - 1 -> l (None at 0)
        self._tier = {}
        self.rows = [a.shape[0] for a in A]

    def levels(self, tier):
        if tier not in self._tier:
            dtype = np.longdouble if tier == "ld" else np.float64
            A, I, P = self._csr
            self._tier[tier] = [Level(A[l], I[l], P[l], dtype) for l in range(self.n_levels)]
        return self._tier[tier]

    # ---- level 0 ---------------------------------------------------------------------------------------------------
    @functools.cached_property
    def _lu0(self):
        import scipy.sparse.linalg as spla

        return spla.splu(self._csr[0][0].tocsc())

    def coarse_exact(self, tier, d):
        if tier == "f64":
            return self._lu0.solve(np.ascontiguousarray(d))
        A0 = self.levels("ld")[0].A
        x = self._lu0.solve(np.asarray(d, dtype=np.float64)).astype(np.longdouble)
        last = np.inf
        for _ in range(8):   # refinement with longdouble residuals, until the residual stops shrinking
            r = d - A0.mv(x)
            now = float(np.abs(r).max())
            if now == 0.0 or now >= 0.5 * last:
                break
            last = now
            x = x + self._lu0.solve(np.asarray(r, dtype=np.float64)).astype(np.longdouble)
        return x

    @functools.cached_property
    def coarse_spectrum(self):
        """(lambda_min, lambda_max) of A_0 (symmetric positive definite) from a dense eigvalsh"""
        a = self._csr[0][0].toarray()
        assert np.abs(a - a.T).max() <= 8 * U * np.abs(a).max()
        ev = np.linalg.eigvalsh((a + a.T) / 2)
        assert ev[0] > 0
        return float(ev[0]), float(ev[-1])

    # ---- the cycle -------------------------------------------------------------------------------------------------
    def smooth(self, tier, cfg, level, u, rhs, from_zero):
        """one call of the smoother on a level; u, rhs [n] or [n, k]; the result in the tier's dtype"""
        L = self.levels(tier)[level]
        u2, r2 = (np.asarray(a, dtype=L.dtype).reshape(L.n, -1) for a in (u, rhs))
        return L.steps(cfg, level, u2, r2, from_zero).reshape(np.shape(rhs))

    def cycle(self, tier, cfg, defects, coarse):
        """level_v_step from the finest level; defects: per level [n_l, k] (changed); returns the level solutions"""
        Ls = self.levels(tier)
        sol = [None] * self.n_levels
        mut = cfg.mut

        def step(l):
            L = Ls[l]
            if l == 0:
                sol[0] = coarse(defects[0])
                return sol[0]
            d = defects[l]
            u = L.steps(cfg, l, np.zeros_like(d), d, True)
            t = L.A.mv(u)
            if L.I is not None and "drop_edge_out" not in mut:
                t = t + L.I.mv(u)
            defects[l - 1] = defects[l - 1] + L.P.tmv(d - t)
            uc = step(l - 1)
            if L.I is not None and "edge_in_before_prolong" in mut:
                d = d - L.I.tmv(u)
            u = u + L.P.mv(uc)
            if L.I is not None and not ({"edge_in_before_prolong", "drop_edge_in"} & mut):
                d = d - L.I.tmv(u)
            defects[l] = d
            sol[l] = L.steps(cfg, l, u, d, False)
            return sol[l]

        step(self.n_levels - 1)
        return sol

    def _lists(self, cfg):
        g, v = list(self.copy_global), list(self.copy_level)
        if "skip_copy_entry" in cfg.mut:
            g[-1], v[-1] = g[-1][:-1], v[-1][:-1]
        return g, v

    def precondition(self, tier, cfg, src, dst0=None, coarse=None, want_coarse=False):
        """PreconditionMG::vmult on src [n_sys] or [n_sys, k]; dst0: what dst held before (seen only by the mutation that
        does not zero it).  want_coarse=True adds the 2-norms of the level-0 solutions [k]."""
        dtype = np.longdouble if tier == "ld" else np.float64
        s = np.asarray(src, dtype=dtype).reshape(self.n_sys, -1)
        g, v = self._lists(cfg)
        defects = []
        for l in range(self.n_levels):
            d = np.zeros((self.rows[l], s.shape[1]), dtype=dtype)
            d[v[l]] = s[g[l]]
            defects.append(d)
        sol = self.cycle(tier, cfg, defects, coarse or (lambda d: self.coarse_exact(tier, d)))
        dst = np.zeros_like(s)
        if "no_zero_dst" in cfg.mut and dst0 is not None:
            dst = np.array(np.broadcast_to(np.asarray(dst0, dtype=dtype).reshape(self.n_sys, -1), s.shape))
        for l in range(self.n_levels):
            dst[g[l]] = sol[l][v[l]]
        out = dst.reshape(np.shape(src))
        if want_coarse:
            return out, np.sqrt((np.asarray(sol[0], dtype=np.float64) ** 2).sum(axis=0))
        return out

    def dense_M(self, cfg):
        """M as a dense fp64 matrix [n_sys, n_sys]"""
        return self.precondition("f64", cfg, np.eye(self.n_sys))

    def coarse_map(self, cfg):
        """T [n_sys, n_0] (fp64): result = M src + T (u_0 - A_0^-1 d_0); built 256 columns at a time"""
        n0 = self.rows[0]
        T = np.empty((self.n_sys, n0))
        for b in range(0, n0, 256):
            e = np.zeros((n0, min(256, n0 - b)))
            e[np.arange(b, b + e.shape[1]), np.arange(e.shape[1])] = 1.0
            T[:, b:b + e.shape[1]] = self.precondition("f64", cfg, np.zeros((self.n_sys, e.shape[1])), coarse=lambda d: e)
        return T

    @functools.lru_cache(maxsize=None)
    def coarse_map_norm(self, cfg):
        """||T||_2: the square root of lambda_max(T^T T) (dense eigvalsh on n_0 x n_0; the largest eigenvalue of a Gram
        matrix is accurate to a few u, relatively)"""
        T = self.coarse_map(cfg)
        return float(np.sqrt(np.linalg.eigvalsh(T.T @ T)[-1]))

    def cg_allowance(self, cfg, tau):
        return tau / self.coarse_spectrum[0] * self.coarse_map_norm(cfg)

    def cg_floor(self):
        """the absolute residual the level-0 CG can reach for a defect of norm 1: u kappa_2(A_0) times a factor of 64 for
        the recurrence's drift -- the tightened tau of the tests is this, scaled by the defect"""
        lo, hi = self.coarse_spectrum
        return 64.0 * U * hi / lo

    def direct_allowance(self, cfg, shape, coarse_norm):
        """the bound of tests/fastdiag_reference.py on ||u_0 - A_0^-1 d_0||_2, c u kappa_2 ||A_0^-1 d_0||_2, through T.  c is
        that file's; kappa_2 here is that of the whole A_0 (coarse_spectrum), which is no smaller than the interior block's
        that fastdiag_reference uses: the boundary rows are diagonal, their eigenvalues |K_e(c, c)| lie inside the interior
        block's spectrum or widen it"""
        import fastdiag_reference as F

        lo, hi = self.coarse_spectrum
        return F.problem(tuple(shape)).c * U * (hi / lo) * np.asarray(coarse_norm) * self.coarse_map_norm(cfg)


# ------------------------------------------------------------------------------------------------ spread and tolerance

def norm2(x):
    """2-norm per column as fp64"""
    x = np.asarray(x)
    return np.asarray(np.sqrt((x * x).sum(axis=0)), dtype=np.float64)


def spread(f64, ld):
    """max over the columns of ||f64 - ld||_2 / ||ld||_2, no smaller than u (the rounding of ld to fp64 alone)"""
    f, l = (np.asarray(a).reshape(np.shape(a)[0], -1) for a in (f64, ld))
    den = norm2(l)
    rel = np.where(den > 0, norm2(f.astype(np.longdouble) - l) / np.where(den > 0, den, 1.0), 0.0)
    return max(U, float(rel.max()))


def tolerance(S_case, ref, allowance=0.0):
    """per column: TOL_FACTOR S_case ||ref||_2 + allowance"""
    return TOL_FACTOR * S_case * norm2(ref) + allowance


def as_f64(x):
    return np.asarray(x, dtype=np.float64)
