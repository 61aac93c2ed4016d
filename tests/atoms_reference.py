"""Independent references for the atom-side kernels (DESIGN.md sections 9 and 10): the pair sums, the exact free-space
potential and its gradient, a cell's error in the energy norm, and the field of a trilinear FE function found by a
brute-force search over the active cells.  Written from the definitions in DESIGN.md, not from csrc/gmg_forces.hpp or
csrc/gmg_exact.hpp.  Two tiers: mpmath at 50 digits on sampled outputs, and an fp64 numpy restatement on all outputs.
Plain helper: no fixtures, no tests.

The tolerance comes from the reference alone, never from what the kernels return.  An output is a sequential sum of n
addends t_j; with u = 2^-53

    |computed - exact| <= u * sum_j (n + C_j) M_j   (+ n * 2^-1022 where an addend may underflow)

n u sum|t_j| is the bound of recursive summation.  C_j bounds the relative error of addend j in units of u and M_j is the
magnitude it is relative to (|t_j|, or for the closed form of the gradient the magnitudes of its two cancelling terms).
With one C for all addends this is (n + C) u S, S = sum M_j.  The C_j are derived by propagating through the addend:

  every + - * / and sqrt is correctly rounded: relative error u (HIP's fp64 division and sqrt without fast math, IEEE
  on the host); erf and erfc 16 ulp, exp 3 ulp (the OpenCL fp64 limits the ROCm device library is built to; glibc is
  within 1 ulp); 1 ulp <= 2 u.

  d = x_i - x_j per coordinate: u.  r2 = dx dx + dy dy + dz dz: 3 u per square, 2 u for the two sums of positive terms,
  5 u.  r = sqrt(r2): 2.5 u + u = 3.5 u.  s = r / r_c: 4.5 u.

  short-range law, f = qq (erfc(s) / r2 + c2 exp(-r2 / r_c^2) / r) / r with c2 = 2 / (sqrt(pi) r_c) (3.5 u):
    erfc(s): the argument error is amplified by |d ln erfc / d ln s| = 2 s e^{-s^2} / (sqrt(pi) erfc s) <= 2 s^2 + 1,
      so (2 s^2 + 1) 4.5 u + 32 u;  erfc / r2: + 6 u                               -> (9 s^2 + 42.5) u
    exp(-r2 / r_c^2): argument 7 u, amplified by s^2, + 6 u;  c2 * . / r: + 9 u     -> (7 s^2 + 15) u
    sum of two positive terms: the larger of the two + u;  / r: + 4.5 u;  qq (u) * . : + 2 u;  * d: + 2 u
    C_force = 9 s^2 + 52;   energy qq erfc(s) / r: (9 s^2 + 36.5) + 2 + 4.5  ->  C_energy = 9 s^2 + 43
  direct law, f = qq / (r2 r): 5 + 3.5 + 1 (product) + 1 (qq) + 1 (division) + 2 (times d) -> C = 14;  qq / r -> C = 6
  potential q erf(s) / r: erf is well conditioned (d ln erf / d ln s <= 1): 4.5 + 32, / r: 4.5, q: 1  ->  C = 42
  gradient of the potential, closed form f = q (A - B) / r^2, A = 2 r e^{-s^2} / (sqrt(pi) r_c), B = erf s, times d / r:
    A: 2 r (3.5), s s (10 u, amplified by s^2 in exp), exp 6, product 1, inv 3.5, product 1 -> (15 + 10 s^2) u |A|
    B: 36.5 u |B|;  the difference adds u |A - B| <= u (|A| + |B|);  / (r r): 9;  q: 1;  d: 2;  / r: 4.5
    -> u [ (15 + 10 s^2) |A| + 36.5 |B| + 18 (|A| + |B|) ] |q| |d| / r^3
    A and B agree to O(s^2) for small s: (|A| + |B|) / |A - B| ~ 3 / s^2, the cancellation of DESIGN.md section 10.
  gradient close to the atom (s <= NEAR_S = 0.1, the sharper requirement): relative to the addend itself,
    |q g(s)| / r_c^2 with g(s) = (2 s e^{-s^2} / sqrt(pi) - erf s) / s^2 = O(s), to a few ulp: a polynomial in s^2
    (3 u: its terms fall off by s^2 <= 0.01 each) times s (4.5 + 1), the factor 2 / sqrt(pi) (2), q / r_c^2 (3),
    d / r (6.5): 20 u;  C = 24 leaves room for one more operation per factor.
"""
import math

import mpmath as mp
import numpy as np

mp.mp.dps = 50
U = 2.0 ** -53
TINY = 2.0 ** -1022
NEAR_S = 0.1  # below this s = r / r_c the gradient of the potential must be accurate relative to the addend itself
C_PHI, C_GRAD_NEAR, C_DIRECT_F, C_DIRECT_E = 42.0, 24.0, 14.0, 6.0
_erf, _erfc = np.vectorize(math.erf, otypes=[float]), np.vectorize(math.erfc, otypes=[float])


def c_short_force(s):
    return 9.0 * s * s + 52.0


def c_short_energy(s):
    return 9.0 * s * s + 43.0


def mpf(v):
    return mp.mpf(float(v))


# ---------------------------------------------------------------------------------------------------------------- inputs
LO = np.array([-1.3, 0.7, 2.1])  # no coordinate of the generators' boxes is a short binary fraction


def charges(rng, n):
    """continuous, away from 0: +-[0.5, 1.5]"""
    return rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.5, n)


def min_distance(x):
    best = np.inf
    for i0 in range(0, len(x), 512):
        d = x[i0:i0 + 512, None, :] - x[None, :, :]
        r = np.sqrt((d * d).sum(-1))
        r[np.arange(len(r)), i0 + np.arange(len(r))] = np.inf
        best = min(best, float(r.min())) if r.size else best
    return best


def thin(x, dmin, keep_first=0):
    """drop every atom closer than dmin to an earlier one (the first keep_first atoms are placed by hand and stay)"""
    keep = np.ones(len(x), bool)
    for i in range(max(keep_first, 1), len(x)):
        d = x[:i][keep[:i]] - x[i]
        if ((d * d).sum(-1) < dmin * dmin).any():
            keep[i] = False
    return keep


def fill(rng, n, sampler, dmin, first=None):
    """n atoms from sampler(m) -> [m, 3], thinned to a least distance dmin; `first` are atoms placed by hand"""
    x = np.zeros((0, 3)) if first is None else np.asarray(first, float).reshape(-1, 3)
    k = len(x)
    while True:
        x = np.vstack([x, sampler(2 * n + 8)])
        x = x[thin(x, dmin, k)]
        if len(x) >= n:
            return x[:n].copy()


def gas(seed, n, r_c, density=1.0):
    """uniform gas of `density` atoms per r_c^3"""
    rng = np.random.default_rng(seed)
    L = r_c * (max(n, 2) / density) ** (1.0 / 3.0)
    x = fill(rng, n, lambda m: LO + rng.uniform(0.0, L, (m, 3)), 0.05 * r_c)
    return x, charges(rng, n), {}


def cluster_in_gas(seed, r_c, rcut, n_cluster=400, n_gas=300):
    """one bin (edge rcut, bins from the minimum corner LO) with n_cluster atoms inside a gas so thin that most bins are
    empty; marks: the cluster's atoms in ascending order (their slots in the bin: the units' boundaries)"""
    rng = np.random.default_rng(seed)
    box = 14
    corner = LO + rcut * np.array([3, 2, 4])

    def sampler(m):
        return LO + rng.uniform(0.0, box * rcut, (m, 3))

    xg = fill(rng, n_gas, sampler, 0.05 * r_c, first=[LO])
    xg = xg[~np.all((xg >= corner - 0.1 * rcut) & (xg <= corner + 1.1 * rcut), axis=1)]
    xc = fill(rng, n_cluster, lambda m: corner + rcut * rng.uniform(0.05, 0.95, (m, 3)), 0.02 * r_c)
    x = np.vstack([xg, xc])
    x = x[rng.permutation(len(x))]
    in_cluster = np.nonzero(np.all((x > corner) & (x < corner + rcut), axis=1))[0]
    return x, charges(rng, len(x)), {"marks": in_cluster}


def slab(seed, r_c, rcut, bins, per_bin=12):
    """atoms in bins[0] x bins[1] x bins[2] bins of edge rcut from LO; some bins stay empty"""
    rng = np.random.default_rng(seed)
    nb = np.array(bins)
    first = [LO, LO + rcut * (nb - 0.25)]  # the minimum corner, and an atom in the last bin of every direction
    n = int(per_bin * nb.prod())
    x = fill(rng, n, lambda m: LO + rcut * rng.uniform(0.0, 1.0, (m, 3)) * (nb - 0.2), 0.05 * r_c, first=first)
    if nb.prod() > 8:  # empty the second bin in x
        x = x[~((x[:, 0] >= LO[0] + rcut) & (x[:, 0] < LO[0] + 2 * rcut)) | (np.arange(len(x)) < 2)]
    return x, charges(rng, len(x)), {}


def on_bin_faces(seed, rcut, n=300, bins=4):
    """coordinates lo + k rcut exactly (lo and rcut are short binary fractions): atoms on faces, edges and corners of bins"""
    rng = np.random.default_rng(seed)
    lo = np.array([-2.0, 1.0, 0.5])
    on = rng.uniform(size=(n, 3)) < 0.5
    on[on.all(1), 2] = False  # no two atoms on nodes of the bin lattice: they could be exactly one cutoff apart
    k = np.where(on, rng.integers(0, bins + 1, (n, 3)), rng.integers(0, bins, (n, 3))).astype(float)
    x = lo + rcut * np.where(on, k, k + rng.uniform(0.05, 0.95, (n, 3)))
    assert np.array_equal((x - lo)[on] / rcut, k[on])
    x[0], x[1] = lo, lo + bins * rcut
    x = x[thin(x, 0.02 * rcut, 2)]
    return x, charges(rng, len(x)), {}


def two_far_clusters(seed, r_c, rcut, n_each=60, apart=300):
    """two clusters `apart` bin edges from each other in every direction: more than 2^24 bins of edge rcut"""
    rng = np.random.default_rng(seed)
    a = fill(rng, n_each, lambda m: LO + rcut * rng.uniform(0.0, 3.0, (m, 3)), 0.05 * r_c, first=[LO])
    b = fill(rng, n_each, lambda m: LO + rcut * (apart + rng.uniform(0.0, 3.0, (m, 3))), 0.05 * r_c)
    x = np.vstack([a, b])[rng.permutation(2 * n_each)]
    extent = x.max(0) - x.min(0)
    assert np.prod(np.floor(extent / rcut) + 1) > 2 ** 24
    return x, charges(rng, len(x)), {}


def cutoff_pairs(seed, r_c, rcut, n_gas=60):
    """atoms 0, 1: exactly rcut apart in x (sqrt(fl(rcut^2)) == rcut: not a member); atoms 2, 3: nextafter(rcut, 0) apart
    in z (a member); each pair sits in two neighbouring bins.  special: the two pairs."""
    rng = np.random.default_rng(seed)
    inside = np.nextafter(rcut, 0.0)
    first = np.array([[0.0, 0.0, 0.0], [rcut, 0.0, 0.0], [0.0, 1.7 * rcut, 0.0], [0.0, 1.7 * rcut, inside],
                      [-0.6 * rcut, -0.6 * rcut, -0.6 * rcut]])
    x = fill(rng, n_gas + 5, lambda m: rcut * rng.uniform(-0.6, 2.4, (m, 3)), 0.05 * r_c, first=first)
    assert np.array_equal(x[:5], first) and np.all(x.min(0) == first[4])
    assert math.sqrt((x[0, 0] - x[1, 0]) ** 2) == rcut and math.sqrt((x[2, 2] - x[3, 2]) ** 2) == inside < rcut
    return x, charges(rng, len(x)), {"special": [(0, 1), (2, 3)], "marks": np.arange(4)}


def sample_indices(n, marks=(), blocks=(64, 128, 256), extra=6, seed=0):
    """first and last output, both sides of every tile edge, the marked ones, and a few random ones"""
    idx = {0, n - 1}
    for b in blocks:
        for k in range(b, n + b, b):
            idx.update(i for i in (k - 1, k, k + 1) if 0 <= i < n)
            if len(idx) > 40:
                break
    idx.update(int(i) for i in marks)
    idx.update(int(i) for i in np.random.default_rng(seed).integers(0, n, extra))
    return np.array(sorted(i for i in idx if 0 <= i < n))


# ------------------------------------------------------------------------------------------------------------- pair sums
def _distances(x, i):
    d = x[i] - x
    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return d, np.sqrt(r2)


def members(x, i, rcut):
    """the partners of atom i in ascending order: the fp64 predicate sqrt(fl(r2)) < rcut of the definition"""
    _, r = _distances(x, i)
    m = r < rcut
    m[i] = False
    return np.nonzero(m)[0]


def pair_sums_numpy(x, q, r_c, cutoff, law="short", special=()):
    """All outputs in fp64: F [n, 3], e [n], their bounds, per atom the smallest addend / bound of its member pairs
    (energy; force: the pair's largest component) and the least relative distance of a pair from the cutoff."""
    n = len(q)
    rcut = cutoff * r_c if cutoff > 0 else np.inf
    F, e, bF, be = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 3)), np.zeros(n)
    det_e, det_F, gap, count = np.full(n, np.inf), np.full(n, np.inf), np.full(n, np.inf), np.zeros(n, int)
    skip = {(a, b) for a, b in special} | {(b, a) for a, b in special}
    for i in range(n):
        d, r = _distances(x, i)
        if np.isfinite(rcut):
            g = np.abs(r - rcut) / rcut
            g[[j for (a, j) in skip if a == i] + [i]] = np.inf
            gap[i] = g.min()
        m = r < rcut
        m[i] = False
        j = np.nonzero(m)[0]
        count[i] = len(j)
        if not len(j):
            continue
        d, r, qq = d[j], r[j], q[i] * q[j]
        s = r / r_c
        if law == "short":
            ec = _erfc(s)
            f = qq * (ec / (r * r) + 2.0 / (math.sqrt(math.pi) * r_c) * np.exp(-s * s) / r) / r
            ee, cF, cE = qq * ec / r, c_short_force(s), c_short_energy(s)
        else:
            f, ee, cF, cE = qq / (r * r * r), qq / r, C_DIRECT_F, C_DIRECT_E
        t = f[:, None] * d
        F[i], e[i] = t.sum(0), 0.5 * ee.sum()
        bF[i] = U * ((len(j) + cF)[:, None] * np.abs(t) if np.ndim(cF) else (len(j) + cF) * np.abs(t)).sum(0) + len(j) * TINY
        be[i] = 0.5 * U * ((len(j) + cE) * np.abs(ee)).sum() + len(j) * TINY
        det_e[i] = (0.5 * np.abs(ee)).min() / be[i]
        det_F[i] = (np.abs(t) / bF[i]).max(1).min()
    return dict(F=F, e=e, bound_F=bF, bound_e=be, detect_e=det_e, detect_F=det_F, gap=gap, count=count)


def pair_sums_mp(x, q, r_c, cutoff, idx, law="short"):
    """The sampled outputs at 50 digits: F [k, 3], e [k] and their bounds.  Membership by the fp64 predicate."""
    rcut = cutoff * r_c if cutoff > 0 else np.inf
    rc, c2 = mpf(r_c), 2 / (mp.sqrt(mp.pi) * mpf(r_c))
    F, e, bF, be = np.zeros((len(idx), 3)), np.zeros(len(idx)), np.zeros((len(idx), 3)), np.zeros(len(idx))
    for k, i in enumerate(idx):
        js = members(x, i, rcut)
        xi = [mpf(v) for v in x[i]]
        acc, accb, n = [mp.mpf(0)] * 4, [mp.mpf(0)] * 4, len(js)
        for j in js:
            d = [xi[c] - mpf(x[j, c]) for c in range(3)]
            r = mp.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            qq = mpf(q[i]) * mpf(q[j])
            if law == "short":
                s = r / rc
                ec = mp.erfc(s)
                f, ee = qq * (ec / (r * r) + c2 * mp.exp(-s * s) / r) / r, qq * ec / r
                cF, cE = c_short_force(float(s)), c_short_energy(float(s))
            else:
                f, ee, cF, cE = qq / (r * r * r), qq / r, C_DIRECT_F, C_DIRECT_E
            for c in range(3):
                acc[c] += f * d[c]
                accb[c] += (n + cF) * abs(f * d[c])
            acc[3] += ee
            accb[3] += (n + cE) * abs(ee)
        F[k], e[k] = [float(v) for v in acc[:3]], float(acc[3] / 2)
        bF[k], be[k] = [U * float(v) + n * TINY for v in accb[:3]], 0.5 * U * float(accb[3]) + n * TINY
    return dict(F=F, e=e, bound_F=bF, bound_e=be)


# ------------------------------------------------------------------------------- exact potential of the Gaussian charges
def _g_series(s, terms):
    """g(s) = (2 s e^{-s^2} / sqrt(pi) - erf s) / s^2 = (2 / sqrt(pi)) sum_{k >= 1} (-1)^k 2 k / ((2 k + 1) k!) s^(2 k - 1)"""
    out = np.zeros_like(s)
    for k in range(terms, 0, -1):
        out += (-1) ** k * 2.0 * k / ((2 * k + 1) * math.factorial(k)) * s ** (2 * k - 1)
    return 2.0 / math.sqrt(math.pi) * out


def potential_numpy(x, q, r_c, pts):
    """phi [m], grad [m, 3] and their bounds in fp64.  The gradient's addend is evaluated without the cancellation (series
    in s below 0.5, where 14 terms are exact to 1e-17), so this tier is itself well inside the bound everywhere."""
    m, n = len(pts), len(q)
    phi, grad, bphi, bgrad = np.zeros(m), np.zeros((m, 3)), np.zeros(m), np.zeros((m, 3))
    inv = 1.0 / (math.sqrt(math.pi) * r_c)
    for p in range(m):
        if n == 0:
            break
        d = pts[p] - x
        r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        zero = r == 0.0
        rs = np.where(zero, 1.0, r)
        s = rs / r_c
        B = _erf(s)
        v = np.where(zero, q * 2.0 * inv, q * B / rs)
        phi[p], bphi[p] = v.sum(), U * (n + C_PHI) * np.abs(v).sum()
        A = 2.0 * rs * np.exp(-s * s) * inv
        g = np.where(s < 0.5, _g_series(np.minimum(s, 0.5), 14), (A - B) / (s * s))
        t = np.where(zero, 0.0, q * g / (r_c * r_c))[:, None] * d / rs[:, None]
        near = s <= NEAR_S
        mag_closed = ((15.0 + 10.0 * s * s + 18.0 + n) * np.abs(A) + (36.5 + 18.0 + n) * B) * np.abs(q) / (rs * rs)
        mag = np.where(near, (n + C_GRAD_NEAR) * np.abs(q * g) / (r_c * r_c), mag_closed)
        grad[p], bgrad[p] = t.sum(0), U * (np.where(zero, 0.0, mag)[:, None] * np.abs(d) / rs[:, None]).sum(0)
    return dict(phi=phi, grad=grad, bound_phi=bphi, bound_grad=bgrad)


def potential_mp(x, q, r_c, pts, idx):
    """phi and grad of the sampled points at 50 digits (the closed form loses 2 log10(1 / s) < 20 of them), with bounds"""
    rc, n = mpf(r_c), len(q)
    inv = 1 / (mp.sqrt(mp.pi) * rc)
    phi, grad, bphi, bgrad = np.zeros(len(idx)), np.zeros((len(idx), 3)), np.zeros(len(idx)), np.zeros((len(idx), 3))
    for k, p in enumerate(idx):
        P = [mpf(v) for v in pts[p]]
        v, bv, ga, bg = mp.mpf(0), mp.mpf(0), [mp.mpf(0)] * 3, [mp.mpf(0)] * 3
        for i in range(n):
            d = [P[c] - mpf(x[i, c]) for c in range(3)]
            r = mp.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            qi = mpf(q[i])
            if r == 0:
                t = qi * 2 * inv
                v, bv = v + t, bv + abs(t)
                continue
            s = r / rc
            A, B = 2 * r * mp.exp(-s * s) * inv, mp.erf(s)
            t = qi * B / r
            v, bv = v + t, bv + abs(t)
            f = qi * (A - B) / (r * r)
            if s <= NEAR_S:
                mag = (n + C_GRAD_NEAR) * abs(f)
            else:
                sf = float(s)
                mag = ((15.0 + 10.0 * sf * sf + 18.0 + n) * abs(A) + (36.5 + 18.0 + n) * B) * abs(qi) / (r * r)
            for c in range(3):
                ga[c] += f * d[c] / r
                bg[c] += mag * abs(d[c]) / r
        phi[k], bphi[k] = float(v), U * (n + C_PHI) * float(bv)
        grad[k], bgrad[k] = [float(a) for a in ga], [U * float(b) for b in bg]
    return dict(phi=phi, grad=grad, bound_phi=bphi, bound_grad=bgrad)


def potential_points(seed, x, r_c, n_uniform=150):
    """uniform points around the atoms, the far field (10^3 r_c away), points on atoms, and points 2e-10 ... 0.1 r_c from
    an atom in random directions.  Returns the points and the index range of the near ones."""
    rng = np.random.default_rng(seed)
    lo, hi = x.min(0) - r_c, x.max(0) + r_c
    uni = rng.uniform(lo, hi, (n_uniform, 3))
    u = rng.normal(size=(12, 3))
    far = x.mean(0) + 1e3 * r_c * u / np.linalg.norm(u, axis=1)[:, None]
    pick = rng.integers(0, len(x), 6)
    scales = [2e-10] + [10.0 ** k for k in range(-9, -1)] + [0.1]
    near = []
    for sc in scales:
        for a in rng.integers(0, len(x), 3):
            v = rng.normal(size=3)
            near.append(x[a] + sc * r_c * v / np.linalg.norm(v))
    pts = np.vstack([uni, far, x[pick], np.array(near)])
    return pts, (len(uni) + len(far) + len(pick), len(pts))


# --------------------------------------------------------------------------------------------- error in the energy norm
def gauss_rule(n1):
    """tensor Gauss rule on the unit cell with n1^3 points (x fastest), and the gradients of the 8 trilinear shape
    functions (vertex a = bx + 2 by + 4 bz) at them: qp [nq, 3], w [nq], sg [nq, 8, 3]"""
    t, w1 = np.polynomial.legendre.leggauss(n1)
    t, w1 = 0.5 * (t + 1.0), 0.5 * w1
    qp = np.array([[t[i], t[j], t[k]] for k in range(n1) for j in range(n1) for i in range(n1)])
    w = np.array([w1[i] * w1[j] * w1[k] for k in range(n1) for j in range(n1) for i in range(n1)])
    sg = np.zeros((len(w), 8, 3))
    for a in range(8):
        for d in range(3):
            v = np.ones(len(w))
            for e in range(3):
                bit = (a >> e) & 1
                v = v * ((1.0 if bit else -1.0) if e == d else (qp[:, e] if bit else 1.0 - qp[:, e]))
            sg[:, a, d] = v
    return qp, w, sg


def quadrature_points(lo, h, qp):
    """the definition's points: fl(lo + fl(h qp)) per coordinate, [n_cells, nq, 3]"""
    return lo[:, None, :] + h[:, None, None] * qp[None, :, :]


def cell_err2_from_gradients(u, dofs, h, w, sg, ga, bga, mpm=False):
    """cell_err2 [n_cells] and its bound from grad phi at the quadrature points (ga [n_cells, nq, 3], absolute bound bga).
    Per point delta = grad phi_h - ga with grad phi_h = sum_a u_a sg_a / h (8 addends of two operations each: absolute error
    10 u sum|.|); (delta + E)^2 - delta^2 <= 2 |delta| E to first order, E = bga + 10 u sum|.| + u |delta|; the products
    with w h^3 (4 u), the sum of 3 squares (3 u) and of nq points (nq u) are relative to the non-negative result."""
    nq = len(w)
    if mpm:
        out, bound = np.zeros(len(h)), np.zeros(len(h))
        for c in range(len(h)):
            tot, tb = mp.mpf(0), mp.mpf(0)
            for k in range(nq):
                for d in range(3):
                    gh = sum(mpf(u[dofs[c, a]]) * mpf(sg[k, a, d]) for a in range(8)) / mpf(h[c])
                    ab = sum(abs(mpf(u[dofs[c, a]]) * mpf(sg[k, a, d])) for a in range(8)) / mpf(h[c])
                    delta = gh - mp.mpf(ga[c][k][d])
                    E = mp.mpf(float(bga[c][k][d])) + 10 * U * ab + U * abs(delta)
                    tot += delta * delta * mpf(w[k]) * mpf(h[c]) ** 3
                    tb += 2 * abs(delta) * E * mpf(w[k]) * mpf(h[c]) ** 3
            out[c], bound[c] = float(tot), float(tb + (nq + 7) * U * tot)
        return out, bound
    uu = u[dofs]  # [n_cells, 8]
    gh = np.einsum("ca,kad->ckd", uu, sg) / h[:, None, None]
    ab = np.einsum("ca,kad->ckd", np.abs(uu), np.abs(sg)) / h[:, None, None]
    delta = gh - ga
    E = bga + 10.0 * U * ab + U * np.abs(delta)
    wh3 = w[None, :] * (h ** 3)[:, None]
    out = ((delta * delta).sum(-1) * wh3).sum(-1)
    return out, ((2.0 * np.abs(delta) * E).sum(-1) * wh3).sum(-1) + (nq + 7) * U * out


# ----------------------------------------------------------------------------- a forest, and the field by brute force
class Forest:
    """A root lattice n0 of cells of edge h0 from `origin`, each cell split into 8 at random down to `depth`, with no 2:1
    balance.  node: the flattening gmg_set_point_locator takes (level by level, roots x fastest; >= 0: the flat index of
    child 0, children a = bx + 2 by + 4 bz contiguous; < 0: active cell -node - 1).  cell_c [n_active, 3], cell_level:
    the integer position and level of the active cells; every cell has its own 8 DoFs 8 cell + vertex."""

    def __init__(self, seed, n0, origin, h0, depth=4, p=0.3):
        rng = np.random.default_rng(seed)
        self.n0, self.origin, self.h0, self.depth = np.array(n0), np.array(origin, float), float(h0), depth
        levels = [[(i, j, k) for k in range(n0[2]) for j in range(n0[1]) for i in range(n0[0])]]
        split = []
        for l in range(depth + 1):
            s = rng.uniform(size=len(levels[l])) < (p if l < depth else 0.0)
            if l == 0:
                s[0] = True  # the first root goes all the way down: cells of every level exist
            elif l < depth and len(s):
                s[0] = True
            split.append(s)
            levels.append([(2 * c[0] + (a & 1), 2 * c[1] + ((a >> 1) & 1), 2 * c[2] + ((a >> 2) & 1))
                           for c, f in zip(levels[l], s) if f for a in range(8)])
        off = np.cumsum([0] + [len(v) for v in levels[:depth + 1]])
        node, cc, cl = [], [], []
        for l in range(depth + 1):
            child = 0
            for c, f in zip(levels[l], split[l]):
                if f:
                    node.append(int(off[l + 1]) + 8 * child)
                    child += 1
                else:
                    node.append(-len(cc) - 1)
                    cc.append(c)
                    cl.append(l)
        self.node = np.array(node, dtype=np.int32)
        self.cell_c, self.cell_level = np.array(cc, dtype=np.int64), np.array(cl, dtype=np.int64)
        self.n_active = len(cc)
        self.active_dofs = np.arange(8 * self.n_active, dtype=np.int32).reshape(-1, 8)
        self.cell_h = self.h0 / 2.0 ** self.cell_level
        self.cell_lo = self.origin + self.cell_h[:, None] * self.cell_c
        self.eps = 2.0 ** -20 * self.h0 / 2 ** depth
        self.hi = self.origin + self.n0 * self.h0

    def face_distance(self, x):
        """least distance in any coordinate of the points x [m, 3] from a plane of the finest level's grid"""
        hf = self.h0 / 2 ** self.depth
        t = (x - self.origin) / hf
        return (np.abs(t - np.round(t)) * hf).min(1)


def _containing_cell(F, pm):
    """index of the one active cell that strictly contains each moved point pm [m, 3]"""
    inside = np.ones((len(pm), F.n_active), bool)
    for d in range(3):
        inside &= (pm[:, d, None] > F.cell_lo[None, :, d]) & (pm[:, d, None] < (F.cell_lo[:, d] + F.cell_h)[None, :])
    assert np.all(inside.sum(1) == 1), "a moved point lies in no cell or in several"
    return inside.argmax(1)


def _factor_bounds(F, cell, x):
    """per coordinate: m = max(|t|, |1 - t|, 1) and the absolute error u (kappa0 + 3 m) of a factor t or 1 - t, where
    t = (x - (origin + h c)) / h: the corner carries u (|h c| + |corner|), which the division by h amplifies"""
    h = F.cell_h[cell][:, None]
    corner = F.cell_lo[cell]
    t = (x - corner) / h
    m = np.maximum(np.maximum(np.abs(t), np.abs(1.0 - t)), 1.0)
    kappa0 = (np.abs(h * F.cell_c[cell]) + np.abs(corner)) / h
    return t, m, kappa0 + 3.0 * m


def field_numpy(F, u, x):
    """phi [m], E [m, 3], their bounds and the number of octants that stay in the lattice [m], by brute force: for octant s
    the point is moved by +-eps per coordinate, the one cell that strictly contains it is searched in the list of active
    cells, and the gradient of that cell's trilinear interpolant is evaluated at the unmoved point.
    Bounds: a product of k factors with absolute errors u e_i and magnitudes <= m_i is off by at most
    u (sum_i e_i prod_{j != i} m_j + (k - 1) prod m); times u_a, summed over 8 vertices (8 u), divided by h, summed over
    the octants (8 u) and divided by their number: 22 u prod m covers those."""
    m = len(x)
    gs, bE, used = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros(m, int)
    for s in range(8):
        sign = np.array([1.0 if (s >> d) & 1 else -1.0 for d in range(3)])
        pm = x + F.eps * sign
        ok = np.all((pm > F.origin) & (pm < F.hi), axis=1)
        if not ok.any():
            continue
        cell = _containing_cell(F, pm[ok])
        t, mm, fe = _factor_bounds(F, cell, x[ok])
        ua = u[F.active_dofs[cell]]
        g, b = np.zeros((ok.sum(), 3)), np.zeros((ok.sum(), 3))
        for d in range(3):
            e1, e2 = [e for e in range(3) if e != d]
            for a in range(8):
                w = (1.0 if (a >> d) & 1 else -1.0)
                for e in (e1, e2):
                    w = w * (t[:, e] if (a >> e) & 1 else 1.0 - t[:, e])
                g[:, d] += w * ua[:, a]
            b[:, d] = np.abs(ua).sum(1) * (fe[:, e1] * mm[:, e2] + fe[:, e2] * mm[:, e1] + 22.0 * mm[:, e1] * mm[:, e2])
        gs[ok] += g / F.cell_h[cell][:, None]
        bE[ok] += b / F.cell_h[cell][:, None]
        used[ok] += 1
    n = np.maximum(used, 1)[:, None]
    E = np.where(used[:, None] > 0, -(gs / n), 0.0)
    pm = np.minimum(np.maximum(x + F.eps, F.origin + F.eps), F.hi - F.eps)
    cell = _containing_cell(F, pm)
    t, mm, fe = _factor_bounds(F, cell, x)
    ua = u[F.active_dofs[cell]]
    phi = np.zeros(m)
    for a in range(8):
        w = np.ones(m)
        for e in range(3):
            w = w * (t[:, e] if (a >> e) & 1 else 1.0 - t[:, e])
        phi += w * ua[:, a]
    bphi = U * np.abs(ua).sum(1) * (fe[:, 0] * mm[:, 1] * mm[:, 2] + fe[:, 1] * mm[:, 0] * mm[:, 2] + fe[:, 2] * mm[:, 0] * mm[:, 1]
                                    + 11.0 * mm.prod(1))
    return dict(phi=phi, E=E, bound_phi=bphi, bound_E=U * bE / n, used=used, phi_cell=cell)


def field_mp(F, u, x, idx):
    """phi and E of the sampled points with the interpolants evaluated at 50 digits (cells from the fp64 search; the
    corner origin + h c is exact here)"""
    phi, E = np.zeros(len(idx)), np.zeros((len(idx), 3))
    org = [mpf(v) for v in F.origin]

    def local(cell, p):
        h = mpf(F.cell_h[cell])
        return h, [(mpf(x[p, d]) - (org[d] + h * int(F.cell_c[cell, d]))) / h for d in range(3)]

    for k, p in enumerate(idx):
        gs, used = [mp.mpf(0)] * 3, 0
        for s in range(8):
            sign = np.array([1.0 if (s >> d) & 1 else -1.0 for d in range(3)])
            pm = x[p:p + 1] + F.eps * sign
            if not np.all((pm > F.origin) & (pm < F.hi)):
                continue
            cell = int(_containing_cell(F, pm)[0])
            h, t = local(cell, p)
            for d in range(3):
                g = mp.mpf(0)
                for a in range(8):
                    w = mp.mpf(1 if (a >> d) & 1 else -1)
                    for e in range(3):
                        if e != d:
                            w *= t[e] if (a >> e) & 1 else 1 - t[e]
                    g += w * mpf(u[F.active_dofs[cell, a]])
                gs[d] += g / h
            used += 1
        E[k] = [float(-(g / used)) if used else 0.0 for g in gs]
        pm = np.minimum(np.maximum(x[p:p + 1] + F.eps, F.origin + F.eps), F.hi - F.eps)
        cell = int(_containing_cell(F, pm)[0])
        h, t = local(cell, p)
        v = mp.mpf(0)
        for a in range(8):
            w = mp.mpf(1)
            for e in range(3):
                w *= t[e] if (a >> e) & 1 else 1 - t[e]
            v += w * mpf(u[F.active_dofs[cell, a]])
        phi[k] = float(v)
    return dict(phi=phi, E=E)


def forest_points(F, seed, n_random=300, n_special=500, ties=True):
    """random interior points; with ties=True (a forest whose planes origin + h c are exact in fp64) also points exactly on
    faces, edges and vertices of cells of every level, on the boundary of the lattice, and outside it by less and by more
    than two root cells"""
    rng = np.random.default_rng(seed)
    pts = [F.origin + rng.uniform(0.0, 1.0, (n_random, 3)) * (F.hi - F.origin)]
    if ties:
        cells = rng.integers(0, F.n_active, n_special)
        lo, h = F.cell_lo[cells], F.cell_h[cells][:, None]
        k = rng.integers(0, 3, (n_special, 3))  # per coordinate: 0 lower plane, 1 upper plane, 2 inside
        k[(k == 2).all(1), 0] = 0
        on = lo + h * np.where(k == 2, rng.uniform(0.05, 0.95, (n_special, 3)), k)
        pts.append(on)
        corners = np.array([[F.origin[d] if (a >> d) & 1 == 0 else F.hi[d] for d in range(3)] for a in range(8)])
        bnd = F.origin + rng.uniform(0.0, 1.0, (60, 3)) * (F.hi - F.origin)
        side = rng.integers(0, 3, 60)
        bnd[np.arange(60), side] = np.where(rng.uniform(size=60) < 0.5, F.origin[side], F.hi[side])
        pts += [corners, bnd]
        for reach in (0.3, 1.9, 2.0, 2.5, 40.0):  # root cells beyond the lattice
            out = F.origin + rng.uniform(0.0, 1.0, (40, 3)) * (F.hi - F.origin)
            side = rng.integers(0, 3, 40)
            sgn = rng.uniform(size=40) < 0.5
            out[np.arange(40), side] = np.where(sgn, F.origin[side] - reach * F.h0, F.hi[side] + reach * F.h0)
            both = rng.uniform(size=40) < 0.3  # beyond the lattice in a second coordinate too
            out[both, (side[both] + 1) % 3] = F.hi[(side[both] + 1) % 3] + reach * F.h0
            pts.append(out)
    return np.vstack(pts)


def ratio(err, bound):
    """the largest error / bound (0 / 0 counts as 0)"""
    err, bound = np.abs(np.asarray(err, float)), np.asarray(bound, float)
    return float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(bound, 1e-320)), initial=0.0))


# ------------------------------------------------------------------------------------------- the cases and their checks
GAS_COUNTS = (1, 2, 63, 64, 65, 257, 1000, 5000)
CUTOFFS = (0, 1.0, 1.5, 2.5, 6)
SLABS = ((5, 1, 1), (1, 5, 1), (1, 1, 5), (2, 2, 2), (3, 3, 3))


def pair_cases():
    """id -> (r_c, cutoff, make) with make() -> (x, q, info).  Cutoffs <= 2.5 are the ones where a single missing pair must
    fail; cutoff 6 and all pairs are kept for the bound only."""
    cases = {}

    def add(name, r_c, cutoff, make):
        cases[f"{name}-rc{r_c}-cut{cutoff}"] = (r_c, cutoff, make)

    def rcut(r_c, cutoff):
        return (cutoff if cutoff > 0 else 2.0) * r_c

    for k, n in enumerate(GAS_COUNTS[:6]):
        for r_c, cutoff in ((0.5, 0), (0.5, 1.5), (0.37, 2.5)):
            add(f"gas{n}", r_c, cutoff, lambda n=n, r_c=r_c, k=k: gas(100 + k, n, r_c))
    for r_c in (0.5, 0.37):
        for cutoff in CUTOFFS:
            add("gas1000", r_c, cutoff, lambda r_c=r_c: gas(110, 1000, r_c))
    add("gas5000", 0.37, 1.0, lambda: gas(111, 5000, 0.37))
    add("gas5000", 0.5, 6, lambda: gas(111, 5000, 0.5))
    for cutoff in (1.0, 2.5, 6, 0):
        add("cluster", 0.37, cutoff, lambda cutoff=cutoff: cluster_in_gas(120, 0.37, rcut(0.37, cutoff)))
    for b in SLABS:
        add("slab%d%d%d" % b, 0.5, 1.5, lambda b=b: slab(130, 0.5, 0.75, b))
    for cutoff in (1.0, 1.5, 2.5):
        add("binfaces", 0.5, cutoff, lambda cutoff=cutoff: on_bin_faces(140, cutoff * 0.5))
    add("farclusters", 0.37, 1.0, lambda: two_far_clusters(150, 0.37, 0.37))
    add("farclusters", 0.5, 2.5, lambda: two_far_clusters(150, 0.5, 1.25))
    for r_c in (0.5, 0.37):
        for cutoff in (1.0, 1.5, 2.5):
            add("cutoffpair", r_c, cutoff, lambda r_c=r_c, cutoff=cutoff: cutoff_pairs(160, r_c, cutoff * r_c))
    return cases


def direct_cases():
    """atom sets of the all-pairs Coulomb sum"""
    cases = {f"gas{n}": (lambda n=n, k=k: gas(100 + k, n, 0.5)) for k, n in enumerate(GAS_COUNTS[:6])}
    cases["gas1000"] = lambda: gas(110, 1000, 0.5)
    cases["gas5000"] = lambda: gas(111, 5000, 0.5)
    cases["cluster"] = lambda: cluster_in_gas(120, 0.37, 0.74)
    return cases


PAIR_CASES, DIRECT_CASES = pair_cases(), direct_cases()
MP_BUDGET = 60000  # pair evaluations of the high-precision tier per case
_cache = {}


def pair_reference(case_id, law="short"):
    """atoms, both tiers and the sampled indices of a case (computed once per process)"""
    key = (case_id, law)
    if key not in _cache:
        if law == "short":
            r_c, cutoff, make = PAIR_CASES[case_id]
        else:
            r_c, cutoff, make = 1.0, 0, DIRECT_CASES[case_id]
        x, q, info = make()
        n = len(q)
        rcut = cutoff * r_c if cutoff > 0 else np.inf
        idx = sample_indices(n, info.get("marks", ()))
        cost = {int(i): len(members(x, i, rcut)) for i in idx}
        keep, spent = [], cost[n - 1]
        for i in idx:  # the last output always; the others in ascending order while the budget lasts
            if i == n - 1 or spent + cost[int(i)] <= MP_BUDGET:
                keep.append(int(i))
                spent += cost[int(i)] if i != n - 1 else 0
        idx = np.array(sorted(set(keep)))
        _cache[key] = dict(x=x, q=q, info=info, r_c=r_c, cutoff=cutoff, idx=idx,
                           np=pair_sums_numpy(x, q, r_c, cutoff, law, info.get("special", ())),
                           mp=pair_sums_mp(x, q, r_c, cutoff, idx, law))
    return _cache[key]


def check_pair_inputs(case_id, R):
    """what the generators promise: no two atoms closer than 1e-3 r_c, no pair within 1e-9 of the cutoff but the two placed
    there, and at cutoffs <= 2.5 every member pair's addend at least 1000 times the tolerance of the output it enters"""
    x, r_c, cutoff, ref = R["x"], R["r_c"], R["cutoff"], R["np"]
    if len(x) > 1:
        assert min_distance(x) >= 1e-3 * r_c
    if cutoff > 0 and len(x) > 1:
        assert ref["gap"].min() >= 1e-9, ref["gap"].min()
    if "special" in R["info"]:
        rcut = cutoff * r_c
        assert 1 not in members(x, 0, rcut) and 0 not in members(x, 1, rcut)  # exactly at the cutoff: excluded
        assert 3 in members(x, 2, rcut) and 2 in members(x, 3, rcut)          # one ulp inside: included
    if 0 < cutoff <= 2.5:
        has = ref["count"] > 0
        assert has.any() or len(x) == 1
        if has.any():
            worst = min(ref["detect_e"][has].min(), ref["detect_F"][has].min())
            print(f"{case_id}: smallest member addend / tolerance {worst:.3g}, members per atom {ref['count'].min()} .. {ref['count'].max()}")
            assert worst >= 1000.0, worst


def check_pair_outputs(what, case_id, R, F, e):
    """F [n, 3], e [n] against both tiers; prints the worst error / bound and returns it"""
    npr, mpr, idx = R["np"], R["mp"], R["idx"]
    assert np.isfinite(F).all() and np.isfinite(e).all()
    rs = dict(F_mp=ratio(F[idx] - mpr["F"], mpr["bound_F"]), e_mp=ratio(e[idx] - mpr["e"], mpr["bound_e"]),
              F_np=ratio(F - npr["F"], npr["bound_F"]), e_np=ratio(e - npr["e"], npr["bound_e"]))
    tiers = max(ratio(npr["F"][idx] - mpr["F"], mpr["bound_F"]), ratio(npr["e"][idx] - mpr["e"], mpr["bound_e"]))
    print(f"{what} {case_id}: error / bound  F {rs['F_mp']:.2e} e {rs['e_mp']:.2e} (mpmath, {len(idx)} atoms)  "
          f"F {rs['F_np']:.2e} e {rs['e_np']:.2e} (numpy, all {len(e)})  numpy vs mpmath {tiers:.2e}")
    assert tiers <= 1.0, "the two tiers of the reference disagree"
    assert max(rs.values()) <= 1.0, rs
    net, total = np.abs(F.sum(0)).max(), np.sqrt((F * F).sum(1)).sum()
    assert net <= 1e-12 * total, (net, total)  # Newton's third law
    return max(rs.values())


# atom sets of the exact potential: counts equal to and one off the block sizes; r_c alternates
POTENTIAL_CASES = {"gas1": (1, 0.5), "gas63": (63, 0.37), "gas64": (64, 0.5), "gas65": (65, 0.37), "gas127": (127, 0.5),
                   "gas128": (128, 0.37), "gas129": (129, 0.5), "gas255": (255, 0.37), "gas256": (256, 0.5),
                   "gas257": (257, 0.37), "gas1000": (1000, 0.5), "cluster": (0, 0.37)}
POINTS_PER_LAUNCH = 7  # the GPU test sets exact_chunk_log2 so that a launch takes about this many points


def potential_reference(key):
    """atoms, points, both tiers; the sampled points: first, last, both sides of the first launch cuts and of the tile
    edges, some of the far field and of the points on atoms, and the points close to an atom"""
    if key not in _cache:
        n, r_c = POTENTIAL_CASES[key]
        x, q, _ = cluster_in_gas(120, 0.37, 0.74) if key == "cluster" else gas(200 + n, n, r_c)
        pts, near = potential_points(300, x, r_c)
        m = len(pts)
        idx = {0, m - 1, 63, 64, 65, 127, 128} | {k * POINTS_PER_LAUNCH + o for k in (1, 2, 9) for o in (-1, 0)}
        idx |= {150, 151, 161, 162, 163, 167}  # far field, on atoms
        budget = max(16, MP_BUDGET // max(len(q), 1))
        base = sorted(i for i in idx if 0 <= i < m)[:budget // 2]
        nearp = list(range(near[0], near[1]))
        idx = np.array(sorted(set(base) | set(nearp[::max(1, -(-len(nearp) // (budget - len(base))))])))
        _cache[key] = dict(x=x, q=q, r_c=r_c, pts=pts, near=near, idx=idx, np=potential_numpy(x, q, r_c, pts),
                           mp=potential_mp(x, q, r_c, pts, idx))
    return _cache[key]


def check_potential_outputs(what, key, R, phi, grad):
    npr, mpr, idx = R["np"], R["mp"], R["idx"]
    assert np.isfinite(phi).all() and np.isfinite(grad).all()
    near = slice(*R["near"])
    rs = dict(phi_mp=ratio(phi[idx] - mpr["phi"], mpr["bound_phi"]), grad_mp=ratio(grad[idx] - mpr["grad"], mpr["bound_grad"]),
              phi_np=ratio(phi - npr["phi"], npr["bound_phi"]), grad_np=ratio(grad - npr["grad"], npr["bound_grad"]),
              grad_near=ratio(grad[near] - npr["grad"][near], npr["bound_grad"][near]))
    tiers = max(ratio(npr["phi"][idx] - mpr["phi"], mpr["bound_phi"]), ratio(npr["grad"][idx] - mpr["grad"], mpr["bound_grad"]))
    print(f"{what} {key}: error / bound  phi {rs['phi_mp']:.2e} grad {rs['grad_mp']:.2e} (mpmath, {len(idx)} points)  "
          f"phi {rs['phi_np']:.2e} grad {rs['grad_np']:.2e} (numpy, all {len(phi)})  near atoms {rs['grad_near']:.2e}  "
          f"numpy vs mpmath {tiers:.2e}")
    assert tiers <= 1.0, "the two tiers of the reference disagree"
    assert max(rs.values()) <= 1.0, rs
    return max(rs.values())


NEAR_DISTANCES = [2e-10] + [10.0 ** k for k in range(-9, -1)] + [0.1]  # in units of r_c
NEAR_DIRECTIONS = 8


def near_atom_case(r_c, seed=7):
    """two atoms (a test may use the first alone) and points at NEAR_DISTANCES r_c from the first in random directions,
    NEAR_DIRECTIONS per distance, ordered by distance"""
    rng = np.random.default_rng(seed)
    x = np.array([[0.31, -1.27, 2.03], [0.31 + 3.0 * r_c, -1.27 + r_c, 2.03]])
    q = np.array([1.0, -0.7])
    v = rng.normal(size=(len(NEAR_DISTANCES), NEAR_DIRECTIONS, 3))
    v /= np.linalg.norm(v, axis=-1)[..., None]
    pts = (x[0] + np.array(NEAR_DISTANCES)[:, None, None] * r_c * v).reshape(-1, 3)
    return x, q, pts


def check_near_atom(what, r_c, x, q, pts, phi, grad):
    """every point against mpmath; prints error / bound per distance"""
    key = ("near", r_c, len(q))
    if key not in _cache:
        _cache[key] = potential_mp(x, q, r_c, pts, np.arange(len(pts)))
    ref = _cache[key]
    k = NEAR_DIRECTIONS
    per = [ratio(grad[i * k:(i + 1) * k] - ref["grad"][i * k:(i + 1) * k], ref["bound_grad"][i * k:(i + 1) * k])
           for i in range(len(NEAR_DISTANCES))]
    print(f"{what}, r_c {r_c}, {len(q)} atom(s): grad error / bound at distance / r_c",
          " ".join(f"{d:g}: {v:.2e}" for d, v in zip(NEAR_DISTANCES, per)))
    assert np.isfinite(grad).all()
    assert ratio(phi - ref["phi"], ref["bound_phi"]) <= 1.0
    assert max(per) <= 1.0, per
    return max(per)


def error_norm_case(n_cells=301, n_atoms=40, r_c=0.37):
    """cells of mixed edge h0 / 2^k, k = 0 .. 4, in random order, each with its own 8 DoFs of a random u, and a gas of atoms
    among them"""
    F = Forest(5, (2, 2, 1), (-1.3, -1.7, -1.1), 0.5, depth=4, p=0.35)
    rng = np.random.default_rng(9)
    cells = rng.permutation(F.n_active)[:n_cells]
    assert len(cells) == n_cells
    assert set(F.cell_level[cells]) == {0, 1, 2, 3, 4}
    x, q, _ = gas(401, n_atoms, r_c, density=n_atoms / (2.0 * (0.5 / r_c) ** 3))
    x = x - x.min(0) + F.origin
    return dict(lo=F.cell_lo[cells], h=F.cell_h[cells], dofs=np.arange(8 * len(cells), dtype=np.int32).reshape(-1, 8),
                u=rng.normal(size=8 * len(cells)), x=x, q=q, r_c=r_c)


def error_norm_reference(E, n1, sample):
    """cell_err2 of all cells in numpy with its bound, of the sampled cells at 50 digits, and the rule"""
    key = ("error norm", n1, tuple(int(i) for i in sample))
    if key not in _cache:
        qp, w, sg = gauss_rule(n1)
        pts = quadrature_points(E["lo"], E["h"], qp)
        g = potential_numpy(E["x"], E["q"], E["r_c"], pts.reshape(-1, 3))
        ce, bound = cell_err2_from_gradients(E["u"], E["dofs"], E["h"], w, sg, g["grad"].reshape(pts.shape), g["bound_grad"].reshape(pts.shape))
        sub = pts[sample].reshape(-1, 3)
        gm = potential_mp(E["x"], E["q"], E["r_c"], sub, np.arange(len(sub)))
        cem, boundm = cell_err2_from_gradients(E["u"], E["dofs"][sample], E["h"][sample], w, sg, gm["grad"].reshape(len(sample), -1, 3),
                                               gm["bound_grad"].reshape(len(sample), -1, 3), mpm=True)
        _cache[key] = dict(qp=qp, w=w, sg=sg, cell_err2=ce, bound=bound, sample=np.asarray(sample), mp=cem, bound_mp=boundm)
    return _cache[key]
