"""The fourth-kind Chebyshev smoother and the Lanczos bound of lambda_max(D^-1 A), written from their definitions (DESIGN.md
section 30; Lottes, Optimal polynomial smoothers for multigrid V-cycles, 2022).  Nothing here is taken from csrc/: the device runs
the three-term recurrence through its product kernels, the reference below also evaluates the polynomial through its roots and
through an eigen-decomposition.  The conventions are those of tests/mg_reference.py (section 16), which this file imports as it
is: two tiers "f64" and "ld", the spread of the tiers is the rounding scale of a case, tolerance = TOL_FACTOR x scale x ||ref||.

    start       r_i = ((uint32)((i + 1) 2654435761) >> 8) 2^-24 - 0.5, i from 0: integers in numpy, every entry an exact double
    Lanczos     B = D^-1.  z = B r, p = z, rho_0 = r.z;  step j:  q = A p, alpha_j = rho_j / p.q, r -= alpha_j q, z = B r,
                rho_{j+1} = r.z, beta_j = rho_{j+1} / rho_j, p = z + beta_j p.
                Breakdown: rho_j or p.q not finite or not positive, or rho_{j+1} not finite: step j does not count;
                rho_{j+1} <= 2^-100 rho_0: step j counts and is the last.
    T           T_jj = 1 / alpha_j + beta_{j-1} / alpha_{j-1},  T_{j,j+1} = sqrt(beta_j) / alpha_j;  ritz = its largest eigenvalue
    bound       lambda = the user's, else min(safety ritz, gershgorin) with the Lanczos source (gershgorin alone after 0 steps), else
                gershgorin
    fourth kind S = q(B A) B,  1 - x q(x) = W_k(1 - 2 x / lambda) / (2 k + 1),  W_k(cos t) = sin((k + 1/2) t) / sin(t / 2):
                  recurrence (f64)  d = 4 / (3 lambda) B r, y = d;  d = (2j-1)/(2j+3) d + (8j+4)/((2j+3) lambda) B (r - A y), y += d
                  roots (ld)        1 - x q(x) = prod_j (1 - x / x_j),  x_j = lambda (1 - cos(j pi / (k + 1/2))) / 2,  j = 1 .. k
                  eigen (f64)       cheb4_by_eig: q on the eigenvalues of D^-1/2 A D^-1/2, W_k by W_{n+1} = 2 t W_n - W_{n-1}

MUTATIONS4 are the wrong derivations the tests must be able to see."""
import functools
from dataclasses import dataclass, field, replace

import numpy as np

import mg_reference as R

CHEB4 = 3                      # Config.kind of the fourth-kind smoother (mg_reference has 0, 1, 2)
GERSHGORIN, LANCZOS = 0, 1
MUTATIONS4 = (
    "first_kind_alpha0",       # the first-kind recurrence on [0, lambda]
    "no_four_thirds",          # the first step without its 4 / 3
    "j_shift",                 # j + 1 in place of j in the two fractions
    "no_safety",               # the Ritz value taken as the bound
)


@dataclass(frozen=True)
class Config4(R.Config):
    kind: int = CHEB4
    source: int = GERSHGORIN
    lanczos_steps: int = 10
    safety: float = 1.2
    mut4: frozenset = field(default_factory=frozenset)

    def with_mut4(self, *names):
        assert all(n in MUTATIONS4 for n in names)
        return replace(self, mut4=frozenset(names))

    def label(self):
        src = f"l{self.lmax:g}" if self.lmax > 0 else ("lanczos" if self.source == LANCZOS else "gershgorin")
        return f"cheb4-s{self.steps}-k{self.degree}-{src}"


# ------------------------------------------------------------------------------------------------ the Lanczos bound

def start_vector(n):
    i = np.arange(1, n + 1, dtype=np.uint64)
    h = (i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return (h >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 - 0.5


def lanczos(L, m):
    """(alpha [m'], beta [m']) in the dtype of the mg_reference.Level L"""
    dt = L.dtype
    r = start_vector(L.n).astype(dt)[:, None]
    diag = L.diag[:, None]
    z = r / diag
    p = z.copy()
    rho = rho0 = (r * z).sum()
    alpha, beta = [], []
    for _ in range(m):
        q = L.A.mv(p)
        pq = (p * q).sum()
        if not (np.isfinite(rho) and np.isfinite(pq) and rho > 0 and pq > 0):
            break
        a = rho / pq
        r = r - a * q
        z = r / diag
        rho1 = (r * z).sum()
        if not np.isfinite(rho1):
            break
        alpha.append(a)
        beta.append(rho1 / rho)
        if rho1 <= dt(2.0) ** -100 * rho0:
            break
        p = z + beta[-1] * p
        rho = rho1
    return np.array(alpha, dtype=dt), np.array(beta, dtype=dt)


def tridiagonal(alpha, beta):
    m = len(alpha)
    T = np.zeros((m, m), dtype=np.float64)
    for j in range(m):
        T[j, j] = 1 / alpha[j] + (beta[j - 1] / alpha[j - 1] if j > 0 else 0)
        if j + 1 < m:
            T[j, j + 1] = T[j + 1, j] = np.sqrt(beta[j]) / alpha[j]
    return T


def ritz(alpha, beta):
    return float(np.linalg.eigvalsh(tridiagonal(alpha, beta))[-1]) if len(alpha) else 0.0


def bound(cfg, gershgorin, ritz_value, steps_run):
    if cfg.lmax > 0:
        return float(cfg.lmax)
    if cfg.source == LANCZOS and steps_run > 0:
        s = (1.0 if "no_safety" in cfg.mut4 else cfg.safety) * ritz_value
        return min(s, gershgorin) if gershgorin > 0 else s
    return float(gershgorin)


# ------------------------------------------------------------------------------------------------ the smoother

class Level4(R.Level):
    """mg_reference.Level with the fourth-kind operator as kind CHEB4"""

    @functools.lru_cache(maxsize=None)
    def lanczos(self, m):
        return lanczos(self, m)

    def lam(self, cfg):
        a, b = self.lanczos(cfg.lanczos_steps) if (cfg.source == LANCZOS and cfg.lmax <= 0) else ((), ())
        return bound(cfg, self.gershgorin, ritz(a, b), len(a))

    def cheb4(self, cfg, r):
        lam, k = self.dtype(self.lam(cfg)), int(cfg.degree)
        diag = self.diag[:, None]
        z = r / diag
        if self.dtype is not np.float64 and not cfg.mut4 - {"no_safety"}:
            ld = np.longdouble
            pi = ld("3.14159265358979323846264338327950288")
            j = np.arange(1, k + 1).astype(ld)
            y = np.zeros_like(r)
            for x in lam * (1 - np.cos(j * pi / (k + ld(0.5)))) / 2:
                y = y + (z - self.A.mv(y) / diag) / x
            return y
        if "first_kind_alpha0" in cfg.mut4:   # Ifpack's recurrence with alpha = 0: theta = lambda / 2, delta = 2 / lambda
            theta, delta = lam / 2, 2 / lam
            s1 = theta * delta
            rhok = 1 / s1
            d = z / theta
            y = d.copy()
            for _ in range(1, k):
                rhokp1 = 1 / (2 * s1 - rhok)
                d = rhokp1 * rhok * d + 2 * rhokp1 * delta * (r - self.A.mv(y)) / diag
                rhok = rhokp1
                y = y + d
            return y
        d = (1 if "no_four_thirds" in cfg.mut4 else self.dtype(4) / 3) / lam * z
        y = d.copy()
        for j in range(1, k):
            i = j + 1 if "j_shift" in cfg.mut4 else j
            d = self.dtype(2 * i - 1) / (2 * i + 3) * d + self.dtype(8 * i + 4) / ((2 * i + 3) * lam) * (r - self.A.mv(y)) / diag
            y = y + d
        return y

    def S(self, cfg, level, r):
        return self.cheb4(cfg, r) if cfg.kind == CHEB4 else super().S(cfg, level, r)


def cheb4_by_eig(A, lam, degree, r):
    """q(D^-1 A) D^-1 r through the eigen-decomposition of D^-1/2 A D^-1/2 (fp64, dense): the third evaluation"""
    a = A.toarray()
    d = np.diag(a).copy()
    assert np.abs(a - a.T).max() <= 8 * R.U * np.abs(a).max()
    ev, V = np.linalg.eigh((a + a.T) / 2 / np.sqrt(d)[:, None] / np.sqrt(d)[None, :])
    t = 1 - 2 * ev / lam
    w0, w1 = np.ones_like(t), 2 * t + 1
    for _ in range(1, degree):
        w0, w1 = w1, 2 * t * w1 - w0
    p = (w1 if degree >= 1 else w0) / (2 * degree + 1)
    q = (1 - p) / ev
    return (V @ (q[:, None] * (V.T @ (r / np.sqrt(d)[:, None])))) / np.sqrt(d)[:, None]


class Hierarchy4(R.Hierarchy):
    """mg_reference.Hierarchy whose levels know the fourth-kind smoother: smooth, cycle and precondition are inherited"""

    def levels(self, tier):
        if tier not in self._tier:
            dtype = np.longdouble if tier == "ld" else np.float64
            A, I, P = self._csr
            self._tier[tier] = [Level4(A[l], I[l], P[l], dtype) for l in range(self.n_levels)]
        return self._tier[tier]


@functools.lru_cache(maxsize=None)
def hierarchy4(name):
    import mg_cases as K

    return Hierarchy4(K.hierarchy(name)[0], name)


# ------------------------------------------------------------------------------------------------ shared references

@functools.lru_cache(maxsize=None)
def lanczos_reference(name, level, m):
    """namespace: alpha, beta, ritz (fp64 of the ld tier), steps_run, and the tolerances made of each quantity's own tier spread"""
    from types import SimpleNamespace

    H = hierarchy4(name)
    (af, bf), (al, bl) = (H.levels(t)[level].lanczos(m) for t in R.TIERS)
    assert len(af) == len(al)
    rf, rl = ritz(af, bf), ritz(al, bl)
    out = SimpleNamespace(alpha=R.as_f64(al), beta=R.as_f64(bl), ritz=rl, steps_run=len(al), gershgorin=H.levels("f64")[level].gershgorin)
    out.S_alpha, out.S_beta = R.spread(af, al), R.spread(bf, bl)
    out.S_ritz = R.spread(np.array([rf]), np.array([rl]))
    out.tol_alpha, out.tol_beta = float(R.tolerance(out.S_alpha, al)), float(R.tolerance(out.S_beta, bl))
    out.tol_ritz = float(R.tolerance(out.S_ritz, np.array([rl])))
    return out


@functools.lru_cache(maxsize=None)
def smoother_reference(name, level, cfg, from_zero):
    """as mg_cases.smoother_reference, for a Config4"""
    from types import SimpleNamespace

    import mg_cases as K

    H = hierarchy4(name)
    u0, rhs = K.smoother_vectors(name, level)
    f, l = (H.smooth(t, cfg, level, u0, rhs, from_zero) for t in R.TIERS)
    S = R.spread(f, l)
    ref = R.as_f64(l)
    ref.setflags(write=False)
    return SimpleNamespace(ref=ref, S=S, tol=float(R.tolerance(S, l)))


@functools.lru_cache(maxsize=None)
def vcycle_reference(name, cfg):
    """as mg_cases.vcycle_reference, for a Config4"""
    from types import SimpleNamespace

    import mg_cases as K

    H = hierarchy4(name)
    src, labels, dst0 = K.vcycle_sources(name)
    f = H.precondition("f64", cfg, src, dst0)
    l, cn = H.precondition("ld", cfg, src, dst0, want_coarse=True)
    S = R.spread(f, l)
    ref = R.as_f64(l)
    ref.setflags(write=False)
    return SimpleNamespace(ref=ref, S=S, tol=R.tolerance(S, l), coarse_norm=cn)
