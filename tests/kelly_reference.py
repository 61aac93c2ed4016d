"""An independent restatement of the error estimator and the refinement marks (gmg_estimate_error, include/gmg_coulomb.h),
written from the definitions in that header alone:

(a) synthetic forests and their face tables: active cells are integer boxes, the neighbours across a face are found by a
    brute-force search over the list of active cells (no tree is walked);
(b) every output in numpy, fp64 / fp32, in the normative operand order -- what the host loop and the device must reproduce
    bit for bit;
(c) the same quadrature sums in mpmath at 50 digits from the same fp64 inputs, with an error bound for (b) derived below
    from the operation count at half an ulp (2^-53) per operation.

Error bound of a face integral.  u = 2^-53.  A corner gradient g = (U1 - U0) / h is two operations.  A jump
g_p[k] - g_m[k] therefore errs by at most 3 u (|g_p[k]| + |g_m[k]|).  The bilinear weights N_k >= 0 (Gauss points lie in
[0, 1]) take at most 6 operations (the coarse side of a sub-face: 0.5 (Q + s) adds one per direction), the product with the
corner value 1, the sum of the terms 3, the difference of the two interpolants of a sub-face 1: with
G = sum_k N_k (|g_p[k]| + |g_m[k]|), |j - j_exact| <= 14 u G and |j| <= G.  j j then errs by (2 * 14 + 1) u G^2, the three
factors gw[q0], gw[q1], measure add 3 u, and the sum over the n = ng^(dim-1) points adds n u: with
S = measure sum_q w_q G_q^2 -- built on the magnitudes of the two cancelling gradients, not on the integral, because the jump
cancels --
    |I - I_exact| <= (32 + n) u S  (+ second-order terms: a factor 1.01),
and a kind-2 slot, the sum of nfc sub-faces, has the sum of their bounds plus nfc u sum S.
Residual term: (4 pi) d, t t, * w, * jxw are 5 operations per point counted relative (t enters twice), the sum nq, diam diam
and the last product 2; all terms are non-negative: |r - r_exact| <= (7 + nq) u r_exact."""
import math
from types import SimpleNamespace

import numpy as np

U53 = 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------- (a) forests
class Forest:
    """Active cells of a forest over n0^dim root cells of edge h0: rows (level, ix, iy, iz) in units of the level's cell size"""

    def __init__(self, dim, n0, h0=1.0, origin=0.0):
        self.dim, self.n0, self.h0, self.origin = dim, n0, h0, origin
        self.cells = [(0,) + tuple(reversed(c)) + (0,) * (3 - dim) for c in np.ndindex(*[n0] * dim)]

    def refine(self, i):
        """replace active cell i by its children (ascending child number, appended at the end)"""
        l, x, y, z = self.cells.pop(i)
        for ch in range(1 << self.dim):
            self.cells.append((l + 1, 2 * x + (ch & 1), 2 * y + ((ch >> 1) & 1), 2 * z + ((ch >> 2) & 1) if self.dim == 3 else 0))
        return self

    def find(self, l, *c):
        c = tuple(c) + (0,) * (3 - len(c))
        return self.cells.index((l,) + c)

    def boxes(self):
        L = max(c[0] for c in self.cells)
        a = np.array(self.cells, dtype=np.int64)
        size = (1 << (L - a[:, 0]))
        lo = a[:, 1:1 + self.dim] * size[:, None]
        return a[:, 0], lo, size, L

    def balance(self):
        """refine until no two cells that share (part of) a face differ by more than one level"""
        while True:
            lv, lo, size, _ = self.boxes()
            worst = None
            for i in range(len(lv)):
                for d in range(self.dim):
                    for side in (0, 1):
                        for j in touching(lo, size, i, d, side, self.dim):
                            if lv[j] > lv[i] + 1:
                                worst = i
            if worst is None:
                return self
            self.refine(worst)


def touching(lo, size, i, d, side, dim):
    """indices of the cells whose boxes share a piece of positive measure of face (d, side) of cell i"""
    plane = lo[i, d] + size[i] if side else lo[i, d]
    m = (lo[:, d] == plane) if side else (lo[:, d] + size == plane)
    for e in range(dim):
        if e != d:
            m &= (lo[:, e] < lo[i, e] + size[i]) & (lo[:, e] + size > lo[i, e])
    return np.nonzero(m)[0]


def inputs(forest, ng=2, nq1=0, fraction=0.6):
    """the arguments of gmg_estimate_error for a forest: cell DoFs by vertex position, levels, the face table, the per-level
    tables, the Gauss rule; nq1 > 0 adds the residual's rule, nq1 points per direction"""
    dim = forest.dim
    nv, nfc, nf = 1 << dim, 1 << (dim - 1), 2 * dim
    lv, lo, size, L = forest.boxes()
    n = len(lv)
    vid, cd = {}, np.zeros((n, nv), dtype=np.int32)
    for a in range(n):
        for v in range(nv):
            key = tuple(int(lo[a, e] + size[a] * ((v >> e) & 1)) for e in range(dim))
            cd[a, v] = vid.setdefault(key, len(vid))
    xyz = np.zeros((len(vid), 3))
    for key, i in vid.items():
        xyz[i, :dim] = forest.origin + forest.h0 / (1 << L) * np.array(key)
    fk, fc = np.zeros((n, nf), dtype=np.uint8), np.zeros((n, nf, nfc), dtype=np.int32)
    inface = [[e for e in range(dim) if e != d] for d in range(dim)]
    for a in range(n):
        for d in range(dim):
            for side in (0, 1):
                f = 2 * d + side
                nb = touching(lo, size, a, d, side, dim)
                if len(nb) == 0:
                    continue
                if len(nb) == 1 and lv[nb[0]] == lv[a]:
                    fk[a, f], fc[a, f, 0] = 1, nb[0]
                elif len(nb) == 1 and lv[nb[0]] == lv[a] - 1:
                    b = nb[0]
                    quad = sum(int((lo[a, e] - lo[b, e]) // size[a]) << k for k, e in enumerate(inface[d]))
                    fk[a, f], fc[a, f, 0], fc[a, f, 1] = 3, b, quad
                elif len(nb) == nfc and all(lv[b] == lv[a] + 1 for b in nb):
                    fk[a, f] = 2
                    for b in nb:
                        quad = sum(int((lo[b, e] - lo[a, e]) // size[b]) << k for k, e in enumerate(inface[d]))
                        fc[a, f, quad] = b
                else:
                    raise ValueError("forest not 2:1 balanced across a face")
    h = forest.h0 / (2.0 ** np.arange(16))
    gx, gw = gauss01(ng)
    out = SimpleNamespace(dim=dim, n_cells=n, n_u=len(vid), cell_dofs=cd, cell_level=lv.astype(np.uint8), face_kind=fk, face_cell=fc,
                          h_of_level=h, face_measure_of_level=h ** (dim - 1), diameter_of_level=h * math.sqrt(dim), jxw_of_level=h ** dim,
                          gauss_x=gx, gauss_w=gw, ng=ng, fraction=fraction, residual=0, nq=0, weight=np.zeros(0), dens=None, vertex_xyz=xyz)
    if nq1:
        x1, w1 = gauss01(nq1)
        w = w1
        for _ in range(dim - 1):
            w = np.multiply.outer(w1, w).reshape(-1)
        out.weight, out.nq = w, len(w)
    return out


def gauss01(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def uniform(dim, n0, h0=1.0):
    return Forest(dim, n0, h0)


def centre_refined(depth=1):
    """3 x 3 x 3 roots, the centre refined; depth 2: one of its children refined again (2:1 balance restored)"""
    f = Forest(3, 3).refine(13)
    if depth == 2:
        f.refine(f.find(1, 2, 2, 2)).balance()
    return f


def random_forest(dim=3, n0=2, depth=3, seed=5):
    rng = np.random.default_rng(seed)
    f = Forest(dim, n0, h0=0.75)
    for level in range(depth):
        cand = [i for i, c in enumerate(f.cells) if c[0] == level]
        for i in sorted(rng.choice(cand, size=max(1, len(cand) // 4), replace=False), reverse=True):
            f.refine(int(i))
    return f.balance()


def solution(inp, kind, seed=1):
    x = inp.vertex_xyz
    if kind == "constant":
        return np.full(inp.n_u, 0.7)
    if kind == "linear":
        return 0.3 + 1.7 * x[:, 0] - 0.9 * x[:, 1] + 0.45 * x[:, 2]
    rng = np.random.default_rng(seed)
    return np.exp(-((x - x.mean(0)) ** 2).sum(1)) * 3.0 + np.sin(2.1 * x[:, 0] + 0.3) * np.cos(1.3 * x[:, 1]) + 0.05 * rng.standard_normal(inp.n_u)


# ------------------------------------------------------------------------------------------------------ (b) numpy, normative
def corner_gradients(inp, u, cells, d):
    """[len(cells), nfc]: (U[v | 1 << d] - U[v]) / h for v ascending over the vertices with bit d clear"""
    nv = 1 << inp.dim
    lo = [v for v in range(nv) if not (v >> d) & 1]
    U = u[inp.cell_dofs[cells]]
    h = inp.h_of_level[inp.cell_level[cells]]
    return np.stack([(U[:, v | (1 << d)] - U[:, v]) / h for v in lo], axis=1)


def interp(c, s, t, dim):
    if dim == 2:
        return c[:, 0] * (1 - s) + c[:, 1] * s
    return c[:, 0] * (1 - s) * (1 - t) + c[:, 1] * s * (1 - t) + c[:, 2] * (1 - s) * t + c[:, 3] * s * t


def quad_sum(inp, jfun, measure):
    s = np.zeros_like(measure)
    for q1 in range(inp.ng if inp.dim == 3 else 1):
        for q0 in range(inp.ng):
            j = jfun(inp.gauss_x[q0], inp.gauss_x[q1] if inp.dim == 3 else 0.0)
            s = s + j * j * inp.gauss_w[q0] * (inp.gauss_w[q1] if inp.dim == 3 else 1.0) * measure
    return s


def sub_face(inp, u, fine, coarse, d, quad):
    dim = inp.dim
    gF, gC = corner_gradients(inp, u, fine, d), corner_gradients(inp, u, coarse, d)
    Q0, Q1 = (quad & 1).astype(np.float64), ((quad >> 1) & 1).astype(np.float64)
    return quad_sum(inp, lambda s, t: interp(gF, s, t, dim) - interp(gC, 0.5 * (Q0 + s), 0.5 * (Q1 + t) if dim == 3 else 0.0, dim),
                    inp.face_measure_of_level[inp.cell_level[fine]])


def face_integrals(inp, u):
    dim, n = inp.dim, inp.n_cells
    nfc = 1 << (dim - 1)
    out = np.zeros((n, 2 * dim))
    for f in range(2 * dim):
        d, side = f >> 1, f & 1
        k1 = np.nonzero(inp.face_kind[:, f] == 1)[0]
        if len(k1):
            nb = inp.face_cell[k1, f, 0]
            m, p = (k1, nb) if side else (nb, k1)
            jump = corner_gradients(inp, u, p, d) - corner_gradients(inp, u, m, d)
            out[k1, f] = quad_sum(inp, lambda s, t: interp(jump, s, t, dim), inp.face_measure_of_level[inp.cell_level[k1]])
        k3 = np.nonzero(inp.face_kind[:, f] == 3)[0]
        if len(k3):
            out[k3, f] = sub_face(inp, u, k3, inp.face_cell[k3, f, 0], d, inp.face_cell[k3, f, 1])
        k2 = np.nonzero(inp.face_kind[:, f] == 2)[0]
        if len(k2):
            s = np.zeros(len(k2))
            for k in range(nfc):
                s = s + sub_face(inp, u, inp.face_cell[k2, f, k], k2, d, np.full(len(k2), k))
            out[k2, f] = s
    return out


def estimate(inp, u, dens=None, residual=None, fraction=None):
    """every output of gmg_estimate_error: namespace(face_int, kelly_sq, residual_sq, eta, threshold, mark, n_marked)"""
    residual = inp.residual if residual is None else residual
    dens = inp.dens if dens is None else dens
    fraction = inp.fraction if fraction is None else fraction
    fi = face_integrals(inp, u)
    diam = inp.diameter_of_level[inp.cell_level]
    acc = np.zeros(inp.n_cells, dtype=np.float32)
    for f in range(2 * inp.dim):
        acc = acc + (diam * fi[:, f]).astype(np.float32)
    eta = np.sqrt(acc)
    assert eta.dtype == np.float32
    rsq = np.zeros(inp.n_cells)
    if residual:
        error = np.zeros(inp.n_cells)
        jxw = inp.jxw_of_level[inp.cell_level]
        for q in range(inp.nq):
            t = 0.0 + 4.0 * math.pi * dens[:, q]
            error = error + t * t * inp.weight[q] * jxw
        rsq = diam * diam * error
        if residual == 1:
            e = eta.astype(np.float64)
            eta = np.sqrt(e * e + diam * diam * error).astype(np.float32)
    mx = np.float32(0) if inp.n_cells == 0 else np.abs(eta).max()
    threshold = fraction * float(mx)
    mark = (np.abs(eta).astype(np.float64) >= threshold).astype(np.uint8)
    return SimpleNamespace(face_int=fi, kelly_sq=acc.astype(np.float64), residual_sq=rsq, eta=eta, threshold=threshold, mark=mark,
                           n_marked=int(mark.sum()))


OUTPUTS = ("face_int", "kelly_sq", "residual_sq", "eta", "mark")


def same_bits(a, b):
    """names of the outputs of two estimates that differ in any bit"""
    bad = [k for k in OUTPUTS if np.ascontiguousarray(getattr(a, k)).tobytes() != np.ascontiguousarray(getattr(b, k)).tobytes()]
    if np.float64(a.threshold).tobytes() != np.float64(b.threshold).tobytes():
        bad.append("threshold")
    if int(a.n_marked) != int(b.n_marked):
        bad.append("n_marked")
    return bad


# ----------------------------------------------------------------------------------------------------- (c) mpmath, 50 digits
def _mp():
    import mpmath

    mpmath.mp.dps = 50
    return mpmath.mpf


def _mp_grad(inp, u, c, d, mpf):
    nv = 1 << inp.dim
    h = mpf(float(inp.h_of_level[inp.cell_level[c]]))
    return [(mpf(float(u[inp.cell_dofs[c, v | (1 << d)]])) - mpf(float(u[inp.cell_dofs[c, v]]))) / h for v in range(nv) if not (v >> d) & 1]


def _mp_weights(s, t, dim):
    return [1 - s, s] if dim == 2 else [(1 - s) * (1 - t), s * (1 - t), (1 - s) * t, s * t]


def _mp_pair(inp, gA, gB, measure, quad, mpf):
    """(integral of (B(gA, s, t) - B(gB, coarse point))^2, S of the bound); quad None: both at (s, t)"""
    dim = inp.dim
    I = S = mpf(0)
    for q1 in range(inp.ng if dim == 3 else 1):
        for q0 in range(inp.ng):
            s, t = mpf(float(inp.gauss_x[q0])), (mpf(float(inp.gauss_x[q1])) if dim == 3 else mpf(0))
            w = mpf(float(inp.gauss_w[q0])) * (mpf(float(inp.gauss_w[q1])) if dim == 3 else 1)
            NA = _mp_weights(s, t, dim)
            NB = NA if quad is None else _mp_weights((((quad & 1) + s) / 2), (((quad >> 1) & 1) + t) / 2, dim)
            j = sum(n * g for n, g in zip(NA, gA)) - sum(n * g for n, g in zip(NB, gB))
            G = sum(n * abs(g) for n, g in zip(NA, gA)) + sum(n * abs(g) for n, g in zip(NB, gB))
            I += j * j * w * measure
            S += G * G * w * measure
    return I, S


def mp_face(inp, u, a, f):
    """(value at 50 digits, error bound of the fp64 restatement) of slot (a, f), both as floats"""
    mpf = _mp()
    dim = inp.dim
    nfc, n = 1 << (dim - 1), inp.ng ** (dim - 1)
    kind, d, side = int(inp.face_kind[a, f]), f >> 1, f & 1
    meas = lambda c: mpf(float(inp.face_measure_of_level[inp.cell_level[c]]))
    if kind == 0:
        return 0.0, 0.0
    if kind == 1:
        b = int(inp.face_cell[a, f, 0])
        I, S = _mp_pair(inp, _mp_grad(inp, u, b, d, mpf), _mp_grad(inp, u, a, d, mpf), meas(a), None, mpf)
        return float(I), float((32 + n) * U53 * 1.01 * S)
    if kind == 3:
        C = int(inp.face_cell[a, f, 0])
        I, S = _mp_pair(inp, _mp_grad(inp, u, a, d, mpf), _mp_grad(inp, u, C, d, mpf), meas(a), int(inp.face_cell[a, f, 1]), mpf)
        return float(I), float((32 + n) * U53 * 1.01 * S)
    gC = _mp_grad(inp, u, a, d, mpf)
    I = S = mpf(0)
    for k in range(nfc):
        F = int(inp.face_cell[a, f, k])
        i, s = _mp_pair(inp, _mp_grad(inp, u, F, d, mpf), gC, meas(F), k, mpf)
        I, S = I + i, S + s
    return float(I), float((32 + n + nfc) * U53 * 1.01 * S)


def mp_residual(inp, dens, a):
    mpf = _mp()
    l = inp.cell_level[a]
    four_pi, jxw, diam = mpf(4.0 * math.pi), mpf(float(inp.jxw_of_level[l])), mpf(float(inp.diameter_of_level[l]))
    e = sum((four_pi * mpf(float(dens[a, q]))) ** 2 * mpf(float(inp.weight[q])) * jxw for q in range(inp.nq))
    r = diam * diam * e
    return float(r), float((7 + inp.nq) * U53 * 1.01 * r)


def mp_eta(inp, u, dens, residual, a):
    """(eta of cell a from the 50-digit sums, a bound for |eta_(b) - eta|): the float accumulation of 2 dim products and
    their conversions errs by (2 dim + 1) 2^-24 relative (all terms are non-negative), the float square root by 2^-24 / 2,
    the fp64 steps of the residual rule are far below that; the face bounds enter through |sqrt(x + dx) - sqrt(x)| <= dx / sqrt(x)
    for 4 dx < x, and <= sqrt(x) + 2 sqrt(dx) otherwise."""
    nf = 2 * inp.dim
    diam = float(inp.diameter_of_level[inp.cell_level[a]])
    parts = [mp_face(inp, u, a, f) for f in range(nf)]
    x, dx = diam * sum(p[0] for p in parts), diam * sum(p[1] for p in parts)
    if residual == 1:
        r, dr = mp_residual(inp, dens, a)
        x, dx = x + r, dx + dr
    eta = math.sqrt(x)
    prop = dx / eta if eta * eta > 4 * dx else eta + 2 * math.sqrt(dx)
    return eta, eta * (nf + 3) * 2.0 ** -24 + prop


def closed_form(inp, c, measure):
    """the integral of a squared bilinear (2D: linear) function with corner values c over a face: measure / 36 c^T M c"""
    M = np.array([[12, 6], [6, 12]]) if inp.dim == 2 else np.array([[4, 2, 2, 1], [2, 4, 1, 2], [2, 1, 4, 2], [1, 2, 2, 4]])
    mpf = _mp()
    cc = [mpf(float(v)) for v in c]
    return float(mpf(float(measure)) / 36 * sum(cc[i] * int(M[i, j]) * cc[j] for i in range(len(cc)) for j in range(len(cc))))
