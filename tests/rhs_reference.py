"""Independent references for the device code between the atom list and the right-hand side: gmg_charge_density and
gmg_rhs_assemble.  Written from the comments on these entry points in include/gmg_coulomb.h, not from csrc/gmg_device.hpp.
Two tiers: mpmath at 50 digits on sampled outputs, and fp64 numpy on all outputs.  Plain helper: no fixtures, no tests.

Densities.  rho(x) = c sum_k q_k exp(-|x - x_k|^2 / r_c^2), c = 4 pi / (r_c^3 pi^1.5), at x = fl(lo + fl(h qp)), over the
atoms on the cell's list.  The device's summation order is unspecified, so this is a bound check; the tolerance comes from
the reference alone.  As in atoms_reference.py, with u = 2^-53 and n addends t_j (any order: (n - 1) u)

    |got - exact| <= u * sum_j (n + C_j) |t_j|  +  n * 2^-1022 * max(1, c max|q|)   (the last where exp underflows)

and C_j follows from the addend t = c * exp(-(r r) * (1 / r_c^2)) * q with every + - * / sqrt correctly rounded (u), exp at
3 ulp = 6 u:
  d = x_k - x per coordinate: u.  r2 = dx dx + dy dy + dz dz: 3 u per square, 2 u for the two sums of positive terms: 5 u.
  r = sqrt(r2): 2.5 + 1 = 3.5 u.  r r: 7 + 1 = 8 u.  1 / r_c^2: 2 u, the product: 1 u  ->  the argument of exp carries 11 u,
  which exp amplifies by the argument itself, s^2 = r^2 / r_c^2: 11 s^2 u.  exp: 6 u.
  c: pi 1 u, r_c^3 2 u, pi^1.5 by pow (16 ulp = 32 u, its argument 1.5 u), product 1 u, division 1 u: 38.5 -> 40 u.
  c * exp * q: 2 u.
  C(s) = 11 s^2 + 48.
The mpmath tier decides membership by the exact predicate (distance to any of the 8 vertices root_lo + {0, root_h}^3 below
cutoff); it leaves out members with s^2 > MP_S2_CUT and adds c sum|q_j| e^-MP_S2_CUT of those to its tolerance, so it stays
a bound.  The numpy tier decides membership by the header's fp64 predicate and carries the same kind of error as the
device, so the device may differ from it by twice the bound; from the mpmath tier by once.

gmg_rhs_assemble.  The header states the arithmetic operation by operation; rhs_numpy restates it and must give the
device's bits.  The mpmath tier sums the same terms exactly; a DoF with k entries e of coefficient c_e, whose slots have
nq quadrature addends t_q (three products each) and m_e Dirichlet terms v_t, is within

    u * sum_e |c_e| (nq + 3 + m_e + k + 1) (sum_q |t_q| + sum_t |v_t|)

of it: (nq + 3) u sum|t_q| for F, one rounding per subtraction on a partial sum below sum|t_q| + sum|v_t|, one for the
product with c_e and k for the sum over the entries.
"""
import math

import mpmath as mp
import numpy as np

import atoms_reference as ar
from atoms_reference import TINY, U, mpf, ratio  # noqa: F401  (ratio: for the tests)

mp.mp.dps = 50
MP_S2_CUT = 60.0
MP_SAMPLES = 200
GAP_ULPS = 64


def c_density(s2):
    return 11.0 * s2 + 48.0


def constant(r_c):
    return 4.0 * math.pi / (r_c * r_c * r_c * math.pi ** 1.5)


# -------------------------------------------------------------------------------------------------------------- densities
def points(cell_lo, cell_h, qp):
    """fl(lo + fl(h qp)) per coordinate: [n_cells, nq, 3]"""
    return cell_lo[:, None, :] + cell_h[:, None, None] * qp[None, :, :]


def _nearest_vertex_distance(rlo, root_h, x):
    """the header's fp64 evaluation for one root corner rlo [3] and atoms x [n, 3]"""
    dl, dh = x - rlo, x - (rlo + root_h)
    m = np.where(np.abs(dl) <= np.abs(dh), dl, dh)
    return np.sqrt(m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1] + m[:, 2] * m[:, 2])


def members_fp64(rlo, root_h, x, cutoff):
    if len(x) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.nonzero(_nearest_vertex_distance(rlo, root_h, x) < cutoff)[0]


def _distance_mp(rlo, root_h, xa):
    """exact distance of one atom to the nearest of the 8 vertices"""
    best = None
    for a in range(8):
        d2 = mp.mpf(0)
        for d in range(3):
            v = mpf(rlo[d]) + (mpf(root_h) if (a >> d) & 1 else 0)
            d2 += (mpf(xa[d]) - v) ** 2
        best = d2 if best is None or d2 < best else best
    return mp.sqrt(best)


def members_exact(rlo, root_h, x, cutoff):
    """the exact predicate; fp64 decides the atoms it cannot get wrong (1e-9 away from the cutoff, its error is 1e-15)"""
    if len(x) == 0:
        return np.zeros(0, dtype=np.int64)
    r = _nearest_vertex_distance(rlo, root_h, x)
    inside = r < cutoff
    for k in np.nonzero(np.abs(r - cutoff) <= 1e-9 * cutoff)[0]:
        inside[k] = _distance_mp(rlo, root_h, x[k]) < mpf(cutoff)
    return np.nonzero(inside)[0]


def cutoff_gap_ulps(root_lo, root_h, x, cutoff):
    """the least |exact distance - cutoff| over all (root cell, atom) pairs in ulps of the cutoff (inf: none within 1e-9)"""
    worst = np.inf
    ulp = mpf(np.spacing(cutoff))
    for rlo in np.unique(root_lo, axis=0):
        if len(x) == 0 or not np.all(np.isfinite(rlo)) or np.abs(rlo).max() > 1e9:
            continue
        r = _nearest_vertex_distance(rlo, root_h, x)
        for k in np.nonzero(np.abs(r - cutoff) <= 1e-9 * cutoff)[0]:
            worst = min(worst, float(abs(_distance_mp(rlo, root_h, x[k]) - mpf(cutoff)) / ulp))
    return worst


def density_numpy(G, use_lists):
    """all outputs in fp64: rho [n_cells, nq], its bound, and the number of atoms on each cell's list"""
    x, q, r_c = G["x"], G["q"], G["r_c"]
    pts = points(G["cell_lo"], G["cell_h"], G["qp"])
    c, inv = constant(r_c), 1.0 / (r_c * r_c)
    nc, nq = pts.shape[:2]
    rho, bound, count = np.zeros((nc, nq)), np.zeros((nc, nq)), np.zeros(nc, dtype=np.int64)
    under = TINY * max(1.0, c * (np.abs(q).max() if len(q) else 0.0))
    for ci in range(nc):
        m = members_fp64(G["root_lo"][ci], G["root_h"], x, G["cutoff"]) if use_lists else np.arange(len(q))
        count[ci] = len(m)
        if not len(m):
            continue
        d = x[m][None, :, :] - pts[ci][:, None, :]
        r = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        s2 = (r * r) * inv
        t = c * np.exp(-s2) * q[m][None, :]
        rho[ci] = t.sum(1)
        bound[ci] = U * ((len(m) + c_density(s2)) * np.abs(t)).sum(1) + len(m) * under
    return dict(rho=rho, bound=bound, count=count)


def density_mp(G, use_lists, idx):
    """the sampled outputs (flat indices cell * nq + q) at 50 digits, with bounds; membership by the exact predicate"""
    x, q, r_c = G["x"], G["q"], G["r_c"]
    pts = points(G["cell_lo"], G["cell_h"], G["qp"])
    nq = pts.shape[1]
    c = 4 * mp.pi / (mpf(r_c) ** 3 * mp.pi ** mp.mpf("1.5"))
    cf, inv, rc2 = float(c), 1.0 / (r_c * r_c), mpf(r_c) ** 2
    xm = [[mpf(v) for v in a] for a in x]
    cq = [c * mpf(v) for v in q]
    under = TINY * max(1.0, cf * (np.abs(q).max() if len(q) else 0.0))
    lists = {}
    rho, bound = np.zeros(len(idx)), np.zeros(len(idx))
    for k, o in enumerate(idx):
        ci, qi = divmod(int(o), nq)
        if ci not in lists:
            lists[ci] = members_exact(G["root_lo"][ci], G["root_h"], x, G["cutoff"]) if use_lists else np.arange(len(q))
        m = lists[ci]
        if not len(m):
            continue
        p = pts[ci, qi]
        d = x[m] - p
        s2f = (d * d).sum(1) * inv  # decides only which addends are bounded instead of evaluated
        P = [mpf(v) for v in p]
        acc, accb = mp.mpf(0), 0.0
        for j, s2j in zip(m, s2f):
            if s2j > MP_S2_CUT + 1e-6:
                continue
            a = xm[j]
            r2 = (a[0] - P[0]) ** 2 + (a[1] - P[1]) ** 2 + (a[2] - P[2]) ** 2
            t = cq[j] * mp.exp(-r2 / rc2)
            acc += t
            accb += (len(m) + c_density(s2j)) * abs(float(t))
        left = s2f > MP_S2_CUT + 1e-6
        accb += ((len(m) + c_density(s2f[left])) * cf * np.abs(q[m][left]) * np.exp(-s2f[left])).sum()
        rho[k] = float(acc)
        bound[k] = U * accb + len(m) * under + cf * np.abs(q[m][left]).sum() * math.exp(-MP_S2_CUT)
    return dict(rho=rho, bound=bound)


def sample(n, seed=0, count=MP_SAMPLES, marks=()):
    """all outputs if there are at most `count`; else the first, the last, the marked and random ones"""
    if n <= count:
        return np.arange(n)
    rng = np.random.default_rng(seed)
    idx = {0, n - 1} | {int(i) for i in marks if 0 <= i < n}
    idx |= {int(i) for i in rng.choice(n, count - len(idx), replace=False)}
    while len(idx) < count:
        idx.add(int(rng.integers(0, n)))
    return np.array(sorted(idx))


def make_cells(rng, n_cells, origin, root_h, k_lo, k_hi, k_out, far=True):
    """n_cells cells of levels 0 .. 3 in roots of the lattice origin + root_h k.  Most roots have k in [k_lo, k_hi) per
    direction; every seventh cell (from the sixth) sits in the root k_out, beyond the atoms by more than the cutoff; the
    last of five or more cells is 10^13 roots away.  Children lie inside a root_lo different from their own corner."""
    lo, h, rlo, outside = np.zeros((n_cells, 3)), np.zeros(n_cells), np.zeros((n_cells, 3)), np.zeros(n_cells, bool)
    for i in range(n_cells):
        k = rng.integers(k_lo, k_hi, 3).astype(float)
        if i % 7 == 5:
            k, outside[i] = np.array(k_out, float), True
        if far and n_cells >= 5 and i == n_cells - 1:
            k, outside[i] = np.array([1e13, -3e13, 2.0]) * (1 if i % 2 else -1), True
        level = i % 4
        rlo[i] = origin + root_h * k
        h[i] = root_h / 2.0 ** level
        child = rng.integers(0, 2 ** level, 3)
        if level and not child.any():
            child[i % 3] = 1
        lo[i] = rlo[i] + h[i] * child
    return lo, h, rlo, outside


def density_geometry(name):
    """id -> atoms, cells and points of a case (r_c alternates; cutoff = 3.5 r_c; root edge 1.7 r_c)"""
    n_atoms, nq, n_cells, seed = DENSITY_CASES[name]
    rng = np.random.default_rng(1000 + seed)
    r_c = 0.5 if seed % 2 else 0.37
    cutoff = 3.5 * r_c
    root_h = 1.7 * r_c
    if name == "cluster":
        x, q, _ = ar.cluster_in_gas(120, r_c, cutoff)
    elif n_atoms == 0:
        x, q = np.zeros((0, 3)), np.zeros(0)
    else:
        x, q, _ = ar.gas(500 + seed, n_atoms, r_c)
    origin = ar.LO - 0.31 * root_h
    box = (x.max(0) - x.min(0)).max() if len(x) else root_h
    k_hi = int(math.ceil((box + cutoff) / root_h)) + 2
    k_out = (k_hi + 4, 1, -2)  # (k_hi + 4) root_h - box - 0.31 root_h > cutoff + 3 root_h
    lo, h, rlo, outside = make_cells(rng, n_cells, origin, root_h, -3, k_hi, k_out)
    qp = rng.uniform(0.0, 1.0, (nq, 3))
    return dict(x=x, q=q, r_c=r_c, cutoff=cutoff, root_h=root_h, cell_lo=lo, cell_h=h, root_lo=rlo, qp=qp, outside=outside)


# name -> (atoms, nq, cells, seed): every atom count, nq and cell count of the list once; 4 k + 1 cells: 5, 9, 13, 41, 33
DENSITY_CASES = {
    "gas1": (1, 1, 1, 1), "gas7": (7, 7, 2, 2), "gas64": (64, 8, 3, 3), "gas65": (65, 9, 5, 4),
    "gas1000-nq27": (1000, 27, 41, 5), "gas1000-nq64": (1000, 64, 13, 6), "gas1000-nq125": (1000, 125, 9, 7),
    "gas20000": (20000, 9, 33, 8), "cluster": (0, 8, 29, 9), "zero": (0, 8, 5, 10),
}
_cache = {}


def density_reference(name, use_lists):
    key = ("density", name, bool(use_lists))
    if key not in _cache:
        if ("geometry", name) not in _cache:
            _cache[("geometry", name)] = density_geometry(name)
        G = _cache[("geometry", name)]
        idx = sample(len(G["cell_h"]) * len(G["qp"]), seed=3)
        _cache[key] = dict(G=G, idx=idx, np=density_numpy(G, use_lists), mp=density_mp(G, use_lists, idx))
    return _cache[key]


def check_density(what, name, use_lists, R, rho):
    """rho [n_cells, nq] against both tiers; prints and returns the worst error / bound"""
    G, npr, mpr, idx = R["G"], R["np"], R["mp"], R["idx"]
    assert rho.shape == npr["rho"].shape and np.isfinite(rho).all()
    flat = rho.reshape(-1)
    r_mp = ratio(flat[idx] - mpr["rho"], mpr["bound"])
    r_np = ratio(rho - npr["rho"], 2.0 * npr["bound"])
    tiers = ratio(npr["rho"].reshape(-1)[idx] - mpr["rho"], mpr["bound"])
    print(f"{what} density {name} lists {int(bool(use_lists))}: error / bound {r_mp:.2e} (mpmath, {len(idx)} outputs) {r_np:.2e} "
          f"(numpy, all {flat.size})  numpy vs mpmath {tiers:.2e}  atoms per list {npr['count'].min()} .. {npr['count'].max()}")
    assert tiers <= 1.0, "the two tiers of the reference disagree"
    assert max(r_mp, r_np) <= 1.0, (r_mp, r_np)
    empty = npr["count"] == 0
    assert np.all(rho[empty] == 0.0) and not np.signbit(rho[empty]).any()  # no atom on the list: exactly +0.0
    if use_lists and len(G["x"]):
        assert empty[G["outside"]].all()
    return max(r_mp, r_np)


def edge_case():
    """Atoms on and next to the cutoff sphere of each of the 8 vertices of the root cell [-0.25, 0.25]^3, cutoff 1.25 =
    3.5 r_c, every coordinate and every difference to a vertex exact in fp64 (|x| < 2).  Per vertex: along one axis at the
    cutoff, one ulp inside, one ulp outside; off the axis by the triple (0.75, 1, 0) = (3, 4, 0) / 4: at the cutoff; with the
    0.75 shortened by 2^-53 (fl(d2) is a tie that rounds back to 1.5625 and the fp64 distance to the cutoff: not a member by
    the header's predicate although the exact distance is below it); shortened and lengthened by 2^-50 (both predicates
    agree); one atom midway between two vertices (the tie of the vertex choice).
    Returns the geometry, the expected membership by the fp64 predicate, and the atoms where the exact one must agree."""
    cutoff, root_h = 1.25, 0.5
    r_c = cutoff / 3.5
    rlo = np.array([-0.25, -0.25, -0.25])
    below, above = np.nextafter(cutoff, 0.0), np.nextafter(cutoff, 2.0)
    short = [0.75, 0.75 - 2.0 ** -53, 0.75 - 2.0 ** -50, 0.75 + 2.0 ** -50]
    x, expect, robust = [], [], []
    for a in range(8):
        v = np.array([0.25 if (a >> d) & 1 else -0.25 for d in range(3)])
        sgn = np.where(v > 0, 1.0, -1.0)
        ax = a % 3
        for dist, inside in ((cutoff, False), (below, True), (above, False)):
            p = v.copy()
            p[ax] = v[ax] + sgn[ax] * dist
            x.append(p); expect.append(inside); robust.append(True)
        b, c = (ax + 1) % 3, (ax + 2) % 3
        for y, inside, rob in zip(short, (False, False, True, False), (True, False, True, True)):
            p = v.copy()
            p[b], p[c] = v[b] + sgn[b] * y, v[c] + sgn[c] * 1.0
            assert p[b] - v[b] == sgn[b] * y
            x.append(p); expect.append(inside); robust.append(rob)
    x.append(np.array([0.0, 1.25, 0.25])); expect.append(True); robust.append(True)  # |dl| = |dh| in x; 1 above the vertex in y
    x = np.array(x)
    rng = np.random.default_rng(77)
    n_cells = 6
    level = np.arange(n_cells) % 3
    h = root_h / 2.0 ** level
    lo = rlo + h[:, None] * np.array([rng.integers(0, 2 ** l, 3) for l in level])
    G = dict(x=x, q=ar.charges(rng, len(x)), r_c=r_c, cutoff=cutoff, root_h=root_h, cell_lo=lo, cell_h=h,
             root_lo=np.tile(rlo, (n_cells, 1)), qp=rng.uniform(0.0, 1.0, (9, 3)), outside=np.zeros(n_cells, bool))
    return G, np.array(expect), np.array(robust)


# ------------------------------------------------------------------------------------------------------- gmg_rhs_assemble
def rhs_numpy(dens, T):
    """the header's arithmetic, operation by operation: rhs [n_dofs] and F [n_slots] after the Dirichlet terms"""
    nc, nq = dens.shape
    nv = 1 << T["dim"]
    shape, w = T["shape"].reshape(nq, nv), T["weight"]
    jxw = T["jxw"][T["cell_level"]][:, None]
    F = np.zeros((nc, nv))
    for k in range(nq):
        F += ((shape[k][None, :] * dens[:, k, None]) * w[k]) * jxw
    F = F.reshape(-1)
    if len(T["term_slot"]):
        np.subtract.at(F, T["term_slot"], T["term_value"])  # unbuffered: one subtraction after the other, t ascending
    ptr, es, ec = T["dof_ptr"], T["entry_slot"], T["entry_coef"]
    val = np.where(ec == 0, F[es], T["coef_table"][ec] * F[es]) if len(es) else np.zeros(0)
    cnt, rhs = np.diff(ptr), np.zeros(len(ptr) - 1)
    for k in range(int(cnt.max()) if len(cnt) else 0):
        sel = np.nonzero(cnt > k)[0]
        rhs[sel] += val[ptr[sel] + k]
    return rhs, F


def rhs_mp(dens, T, idx):
    """the sampled DoFs at 50 digits, with bounds"""
    nq = dens.shape[1]
    nv = 1 << T["dim"]
    shape, w = T["shape"].reshape(nq, nv), T["weight"]
    ts, tv = T["term_slot"], T["term_value"]
    out, bound = np.zeros(len(idx)), np.zeros(len(idx))
    slot_cache = {}

    def slot_value(s):
        if s not in slot_cache:
            cell, i = divmod(s, nv)
            j = mpf(T["jxw"][T["cell_level"][cell]])
            f, a = mp.mpf(0), mp.mpf(0)
            for k in range(nq):
                t = mpf(shape[k, i]) * mpf(dens[cell, k]) * mpf(w[k]) * j
                f, a = f + t, a + abs(t)
            t0, t1 = np.searchsorted(ts, s, "left"), np.searchsorted(ts, s, "right")
            for t in range(t0, t1):
                f, a = f - mpf(tv[t]), a + abs(mpf(tv[t]))
            slot_cache[s] = (f, a, t1 - t0)
        return slot_cache[s]

    for n, d in enumerate(idx):
        e0, e1 = int(T["dof_ptr"][d]), int(T["dof_ptr"][d + 1])
        acc, accb = mp.mpf(0), mp.mpf(0)
        for e in range(e0, e1):
            f, a, m = slot_value(int(T["entry_slot"][e]))
            c = mpf(T["coef_table"][T["entry_coef"][e]]) if T["entry_coef"][e] else mp.mpf(1)
            acc += c * f
            accb += abs(c) * (nq + 3 + m + (e1 - e0) + 1) * a
        out[n], bound[n] = float(acc), U * float(accb)
    return dict(rhs=out, bound=bound)


def term_runs(rng, n_slots, lengths):
    """ascending term slots with runs of the given lengths on distinct random slots, in this order"""
    slots = np.sort(rng.choice(n_slots, len(lengths), replace=False))
    ts = np.repeat(slots, lengths).astype(np.int32)
    return ts, rng.normal(size=len(ts))


RUNS = [300] + [1] * 211 + [2, 3000] + [1] * 40 + [2, 300, 1, 3000]  # 300 from t = 0; 2 over t = 512; 3000 over many; 3000 to the end
DOF_ENTRIES = [0, 1, 8, 40, 3, 0, 2, 5]


def rhs_tables(name):
    """id -> the tables of a case: random shape values, weights, levels 0 .. 15 with distinct JxW, all 256 coefficient codes,
    DoFs with 0, 1, 8 and 40 entries, term runs of length 1, 2, 300 and 3000"""
    dim, nq, n_cells, n_dofs, runs, seed = RHS_CASES[name]
    rng = np.random.default_rng(2000 + seed)
    nv = 1 << dim
    n_slots = n_cells * nv
    T = dict(dim=dim, nq=nq, n_cells=n_cells, shape=rng.normal(size=(nq, nv)), weight=rng.uniform(0.1, 1.0, nq),
             cell_level=(rng.permutation(n_cells) % 16).astype(np.uint8), jxw=8.0 ** -np.arange(16) * rng.uniform(1.0, 2.0, 16),
             coef_table=rng.normal(size=256))
    if runs == "identity":  # DoF d = slot d as it is: F per slot
        cnt = np.ones(n_slots, dtype=np.int64)
        T["entry_slot"], T["entry_coef"] = np.arange(n_slots, dtype=np.int32), np.zeros(n_slots, dtype=np.uint8)
        lengths = [l for l in RUNS if l <= 300][:max(1, n_slots // 2)]
    else:
        cnt = np.array([DOF_ENTRIES[i % len(DOF_ENTRIES)] for i in range(n_dofs)], dtype=np.int64)
        n_ent = int(cnt.sum())
        T["entry_slot"] = rng.integers(0, n_slots, n_ent).astype(np.int32)
        T["entry_coef"] = rng.permutation(np.arange(n_ent) % 256).astype(np.uint8)
        lengths = [] if runs == "none" else RUNS[:n_slots] if runs == "runs" else [300] + [1] * runs + [3000]
    T["dof_ptr"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    if lengths:
        T["term_slot"], T["term_value"] = term_runs(rng, n_slots, lengths)
    else:
        T["term_slot"], T["term_value"] = np.zeros(0, dtype=np.int32), np.zeros(0)
    # the densities come from gmg_charge_density on these cells: a few atoms of both signs, no lists
    x, q, _ = ar.gas(600 + seed, 7, 0.5)
    lo, h, rlo, _ = make_cells(rng, n_cells, ar.LO - 0.2, 0.8, -1, 3, (9, 9, 9), far=False)
    T["geometry"] = dict(x=x, q=q, r_c=0.5, cutoff=1.75, root_h=0.8, cell_lo=lo, cell_h=h, root_lo=rlo, qp=rng.uniform(0.0, 1.0, (nq, 3)))
    return T


GRID_STRIDE = 2048 * 256  # beyond this many cells, terms or DoFs a thread takes more than one
# name -> (dim, nq, cells, DoFs, terms, seed)
RHS_CASES = {
    "d3-nq8": (3, 8, 301, 800, "runs", 1), "d2-nq1": (2, 1, 37, 90, "runs", 2), "d3-nq27": (3, 27, 64, 300, "runs", 3),
    "d2-nq125": (2, 125, 1100, 700, "runs", 4), "d3-nq512": (3, 512, 17, 60, "runs", 5),
    "d3-identity": (3, 8, 45, 0, "identity", 6), "d2-identity": (2, 27, 30, 0, "identity", 7),
    "no-terms": (3, 8, 33, 100, "none", 8), "one-cell": (2, 8, 1, 9, "runs", 9),
    "grid-stride": (3, 1, GRID_STRIDE + 301, GRID_STRIDE + 77, GRID_STRIDE + 5, 10),
}


def rhs_sample(T):
    """the DoFs of the high-precision tier: about MP_SAMPLES, the DoFs on both sides of the grid stride and the last one"""
    n = len(T["dof_ptr"]) - 1
    return sample(n, seed=5, marks=(GRID_STRIDE - 1, GRID_STRIDE, GRID_STRIDE + 1))


# ------------------------------------------------------------------------------------ end to end: the driver's cycle 0
def mesh_from_dofs(X):
    """the root lattice of cycle 0 from the DoF coordinates alone: the sorted coordinates per direction, and the DoF of
    every lattice vertex [nx, ny, nz]"""
    axes = [np.unique(X[:, d]) for d in range(3)]
    n = [len(a) for a in axes]
    assert n[0] * n[1] * n[2] == len(X), "cycle 0 is a full lattice"
    ijk = np.stack([np.searchsorted(axes[d], X[:, d]) for d in range(3)], 1)
    dof = np.full(n, -1, dtype=np.int64)
    dof[ijk[:, 0], ijk[:, 1], ijk[:, 2]] = np.arange(len(X))
    assert (dof >= 0).all()
    return axes, dof


def end_to_end_reference(X, x, q, r_c, cutoff, n1, use_lists):
    """rhs[d] = sum over the cells around d and their n1^3 Gauss points of phi_d(x_q) rho(x_q) w_q h^3, rho over the atoms
    on the cell's list, from the DoF coordinates, the rule and the atoms alone; with its bound.  The addends carry C(s) of
    the density plus 16 u for the shape value, the weight and h^3 (a few ulp each) and for the products, plus
    8 s X u / r_c for a quadrature point that the driver may form 2 ulp of X = max|coordinate| away from ours (an
    absolute error of the point changes s^2 = r^2 / r_c^2 by 2 r delta / r_c^2)."""
    axes, dof = mesh_from_dofs(X)
    qp, w, _ = ar.gauss_rule(n1)
    nq = len(w)
    shape = np.ones((nq, 8))
    for a in range(8):
        for d in range(3):
            shape[:, a] *= qp[:, d] if (a >> d) & 1 else 1.0 - qp[:, d]
    c, inv = constant(r_c), 1.0 / (r_c * r_c)
    rhs, bound = np.zeros(len(X)), np.zeros(len(X))
    h = axes[0][1] - axes[0][0]
    n_add = 8 * nq * len(q)  # addends of a DoF at most
    gap = np.inf  # the least relative distance of an atom from a cutoff sphere
    I, J, K = np.meshgrid(*[np.arange(len(a) - 1) for a in axes], indexing="ij")
    I, J, K = I.reshape(-1), J.reshape(-1), K.reshape(-1)
    for c0 in range(0, len(I), 2048):
        i, j, k = I[c0:c0 + 2048], J[c0:c0 + 2048], K[c0:c0 + 2048]
        lo = np.stack([axes[0][i], axes[1][j], axes[2][k]], 1)
        if use_lists:  # the header's fp64 predicate, for all cells of the chunk at once
            dl, dh = x[None, :, :] - lo[:, None, :], x[None, :, :] - (lo + h)[:, None, :]
            m = np.where(np.abs(dl) <= np.abs(dh), dl, dh)
            dist = np.sqrt(m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1] + m[..., 2] * m[..., 2])
            on = dist < cutoff
            gap = min(gap, float(np.abs(dist - cutoff).min() / cutoff))
            if not on.any():
                continue
        else:
            on = np.ones((len(lo), len(q)), bool)
        pts = lo[:, None, :] + h * qp[None, :, :]
        d = x[None, None, :, :] - pts[:, :, None, :]
        s2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) * inv
        t = np.where(on[:, None, :], c * np.exp(-s2) * q[None, None, :], 0.0)  # [cells, nq, atoms]
        cj = c_density(s2) + 16.0 + 8.0 * np.sqrt(s2) * np.abs(pts).max() / r_c + n_add
        wh3 = w * h ** 3
        for a in range(8):
            dd = dof[i + (a & 1), j + ((a >> 1) & 1), k + ((a >> 2) & 1)]
            np.add.at(rhs, dd, ((shape[:, a] * wh3)[None, :, None] * t).sum((1, 2)))
            np.add.at(bound, dd, ((shape[:, a] * wh3)[None, :, None] * cj * np.abs(t)).sum((1, 2)))
    return rhs, U * bound + n_add * TINY * max(1.0, c * np.abs(q).max()), gap
