"""The hierarchies, smoother configurations, vectors and tolerances that tests/test_mg_reference_cpu.py and
tests/test_gpu_mg_reference.py share.  Everything a bound is made of comes from tests/mg_reference.py."""
import functools
import os
from types import SimpleNamespace

import numpy as np

import mg_reference as R
from gpu_util import pkg
from oracle import gmg_oracle as go
from oracle import step50_oracle as so

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

#        name: (vacuum, mesh, bc, cycle, level rows, edge nnz, copy-list sizes, n_sys, constrained)
ADAPTIVE = {
    "A2": (1, 0.25, "Exact", 1, [729, 490], [0, 1415], [726, 123], 1117, 674),
    "A3": (1, 0.25, "Exact", 3, [729, 1303, 250], [0, 2181, 772], [626, 868, 54], 2008, 1034),
    "B3": (2, 0.5, "Inhomogeneous", 3, [1331, 827, 941], [0, 2642, 3130], [1303, 352, 395], 2794, 1346),
}
NAMES = ("hier3", "A2", "A3", "B3", "SYN")
LAT = "LAT"   # the layout case: not in NAMES, its dense M would have 24389 rows
SMOOTH_LEVELS = [("A2", 1), ("A3", 1), ("A3", 2), ("B3", 1), ("B3", 2), ("SYN", 1)]


def _nnz(m):
    return 0 if m is None else int(m.nnz)


def _adaptive(name):
    vac, mesh, bc, last, rows, edges, copies, n_sys, n_con = ADAPTIVE[name]
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=1, mesh_size=mesh, vacuum=vac, problem="GaussianCharges", dim=3, bc=bc, cycles=last + 1,
                             r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR"))
    p.read_lammps(os.path.join(GOLDEN, "atom_n1_2.data"))
    for cycle in range(last + 1):
        p.run_cycle(cycle, on_device=False)
        h = p.hierarchy()
        if cycle < last:
            p.finish_cycle_with(go.OracleMG(h, smoother=go.SSOR).solve(h.system_rhs, x0=p.vector("initial_guess"))["x"])
    p.close()
    # a drifting mesh must not silently empty the tests
    assert [m.n_rows for m in h.level_matrices] == rows
    assert [_nnz(e) for e in h.edge_matrices] == edges
    assert [len(g) for g in h.copy_global] == copies
    assert h.system_matrix.n_rows == n_sys and int(np.sum(h.constrained)) == n_con
    return h


def _csr_ns(a):
    a = a.tocsr()
    a.sort_indices()
    return SimpleNamespace(n_rows=a.shape[0], n_cols=a.shape[1], nnz=int(a.nnz), rowptr=a.indptr.astype(np.int64),
                           col=a.indices.astype(np.int32), val=a.data.astype(np.float64))


def _synthetic(k=3):
    """two levels, the upper one with 64 k + 17 rows (no multiple of a wavefront, several SSOR blocks), its copy list in
    permuted order, a partial copy list on level 0, an edge matrix on the upper level"""
    import scipy.sparse as sp

    rng = np.random.default_rng(64 * k + 17)
    n1 = 64 * k + 17
    n0 = (n1 + 1) // 2

    def spd(n, extra):
        off = sp.diags([-np.ones(n - 1), -np.ones(n - 1)], [-1, 1])
        i, j = rng.integers(0, n, extra), rng.integers(0, n, extra)
        keep = i != j
        w = sp.coo_matrix((rng.uniform(-0.5, 0.0, keep.sum()), (i[keep], j[keep])), shape=(n, n))
        a = (off + w + w.T).tocsr()
        a.sum_duplicates()
        return (a + sp.diags(np.asarray(abs(a).sum(axis=1)).ravel() * rng.uniform(1.02, 1.3, n))).tocsr()

    A0, A1 = spd(n0, 40), spd(n1, 90)
    rows, cols, vals = [], [], []
    for c in range(n0):
        for r, v in ((2 * c - 1, 0.5), (2 * c, 1.0), (2 * c + 1, 0.5)):
            if 0 <= r < n1:
                rows.append(r); cols.append(c); vals.append(v)
    P = sp.csr_matrix((vals, (rows, cols)), shape=(n1, n0))
    ei, ej = rng.integers(0, n1, 60), rng.integers(0, n1, 60)
    I1 = sp.csr_matrix((rng.uniform(-0.3, 0.3, 60), (ei, ej)), shape=(n1, n1))
    I1.sum_duplicates()
    n_sys = n1 + 20   # 8 entries belong to no list (hanging), 12 to level 0's
    perm = rng.permutation(n_sys)
    g1, v1 = perm[:n1], rng.permutation(n1)
    g0, v0 = perm[n1:n1 + 12], rng.permutation(n0)[:12]
    Ssys = sp.identity(n_sys, format="csr") * 2.0
    constrained = np.zeros(n_sys, dtype=bool)
    constrained[perm[n1 + 12:]] = True
    return SimpleNamespace(system_matrix=_csr_ns(Ssys), system_rhs=rng.standard_normal(n_sys), constrained=constrained,
                           level_matrices=[_csr_ns(A0), _csr_ns(A1)], edge_matrices=[None, _csr_ns(I1)], prolongations=[_csr_ns(P)],
                           copy_global=[g0.astype(np.int32), g1.astype(np.int32)], copy_level=[v0.astype(np.int32), v1.astype(np.int32)])


# tests/test_gpu_context_reuse.py: hierarchies that differ from SYN in ONE thing a context derives
# tables from, and agree with it in every size -- what a context that kept a table of SYN's would not notice by a fault.
REUSE_TWIN = "SYN-T"
REUSE_SUBSTITUTIONS = ("SYN-A1", "SYN-A0", "SYN-I", "SYN-P")
REUSE_NAMES = (REUSE_TWIN,) + REUSE_SUBSTITUTIONS


def _respd(m, seed):
    """m's pattern with other values: the off-diagonal a_ij times s_i s_j, s_i in [0.5, 1) drawn per row (symmetric, and no
    entry grows), then the diagonal set as spd() of _synthetic sets it, sum_j |a_ij| times a factor in [1.02, 1.3) per row:
    symmetric and strictly diagonally dominant with a positive diagonal, hence SPD"""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    a = R._scipy_csr(m).tocoo()
    s = rng.uniform(0.5, 1.0, a.shape[0])
    off = a.row != a.col
    val = np.where(off, a.data * s[a.row] * s[a.col], 0.0)
    rowsum = np.bincount(a.row, weights=np.abs(val), minlength=a.shape[0])
    diag = rowsum * rng.uniform(1.02, 1.3, a.shape[0])
    val = np.where(off, val, diag[a.row])
    out = _csr_ns(sp.csr_matrix((val, (a.row, a.col)), shape=a.shape))
    assert np.array_equal(out.rowptr, m.rowptr) and np.array_equal(out.col, m.col)   # the pattern is m's
    return out


def _reuse_case(name):
    """SYN with one thing replaced (the sizes, and with them everything the signature of the fused copies' tables holds, are SYN's):
    SYN-T   both copy lists redrawn: another assignment of the system entries to level 1 / level 0 / no list, another order
    SYN-A1  A_1 of the same pattern with other values (_respd): invd, the Gershgorin bound and the SSOR records must follow
    SYN-A0  the same on level 0: the coarse CG's operator
    SYN-I   the edge matrix of another pattern
    SYN-P   the prolongation with the weights 0.25 / 1 / 0.25 in place of 0.5 / 1 / 0.5: P^T must follow"""
    import scipy.sparse as sp

    h = SimpleNamespace(**vars(hierarchy("SYN")[0]))
    n0, n1 = (m.n_rows for m in h.level_matrices)
    n_sys = h.system_matrix.n_rows
    if name == "SYN-T":
        rng = np.random.default_rng(7919 + n_sys)
        perm = rng.permutation(n_sys)
        g1, v1 = perm[:n1], rng.permutation(n1)
        g0, v0 = perm[n1:n1 + 12], rng.permutation(n0)[:12]
        h.constrained = np.zeros(n_sys, dtype=bool)
        h.constrained[perm[n1 + 12:]] = True
        h.copy_global, h.copy_level = [g0.astype(np.int32), g1.astype(np.int32)], [v0.astype(np.int32), v1.astype(np.int32)]
    elif name == "SYN-A1":
        h.level_matrices = [h.level_matrices[0], _respd(h.level_matrices[1], 1)]
    elif name == "SYN-A0":
        h.level_matrices = [_respd(h.level_matrices[0], 2), h.level_matrices[1]]
    elif name == "SYN-I":
        rng = np.random.default_rng(3)
        ei, ej = rng.integers(0, n1, 60), rng.integers(0, n1, 60)
        I1 = sp.csr_matrix((rng.uniform(-0.3, 0.3, 60), (ei, ej)), shape=(n1, n1))
        I1.sum_duplicates()
        h.edge_matrices = [None, _csr_ns(I1)]
    elif name == "SYN-P":
        P = R._scipy_csr(h.prolongations[0]).copy()
        P.data = np.where(P.data == 0.5, 0.25, P.data)
        h.prolongations = [_csr_ns(P)]
    else:
        raise KeyError(name)
    return h


LAT_CELLS = (10, 28)   # cells per direction of LAT's level 0 and level 1


def sell_padding(m):
    """(rows, padded entries / nnz) of a SELL-64 copy of m: per slice of 64 rows the widest row, rounded up to a multiple of
    4, times 64.  The library keeps such a copy of an operator with 1024 rows or more whose padding is at most 1.12 (set_csr
    in csrc/gmg_coulomb.hip; a slice that follows a column pattern is as wide as the pattern, which for the operators of LAT
    is the widest row); every other operator stays on the CSR row-window kernel, whatever the layout switches say.  This
    restates the library's rule: should the rule change, the GPU layout tests' assertion that A_1 of LAT reports every layout
    bit is what notices, not this function."""
    w = np.diff(np.asarray(m.rowptr, dtype=np.int64))
    pad = -len(w) % 64
    per_slice = np.concatenate([w, np.zeros(pad, dtype=w.dtype)]).reshape(-1, 64).max(axis=1)
    return int(m.n_rows), float(((per_slice + 3) // 4 * 4 * 64).sum() / m.nnz)


def _lattice_case():
    """LAT: two levels on which every operator of the cycle is regular enough for the SELL-64 layouts, so that the layout
    switches change kernels (they change nothing on A2, A3, B3, SYN and hier3: test_layout_case_qualifies).  Level 1 is the
    constrained Q1 Laplacian of a 29^3 lattice with its full 27-point rows (SELL-64, the pattern-run kernel, row classes and
    the plane-by-plane lattice kernel all take it).  Level 0 is the same operator on 11^3 (1331 rows; its padding keeps it on
    CSR row windows, so the level-0 CG sums in one order under every switch).  The transfer and the edge matrix are synthetic
    but regular: P has 4 entries a row over a window that moves evenly through the coarse indices, so P^T has 72 to 76 a
    row; I_1 is a symmetric circulant with 4 entries a row.  All entries but 8 (in no list: exact zeros) are level 1's."""
    import scipy.sparse as sp

    lat0, lat1 = (so.Lattice(3, n, 0.0, 1.0 / n) for n in LAT_CELLS)
    A0, A1 = (so.assemble_constrained(lat, so.cell_matrices(lat), lat.boundary_mask())[0] for lat in (lat0, lat1))
    n0, n1 = A0.n_rows, A1.n_rows
    i = np.arange(n1, dtype=np.int64)
    cols = ((i * n0) // n1)[:, None] + np.arange(4)[None, :]
    P = sp.csr_matrix((np.tile([0.125, 0.375, 0.375, 0.125], n1), ((np.repeat(i, 4)), (cols % n0).ravel())), shape=(n1, n0))
    off = np.array([-2, -1, 1, 2])
    I1 = sp.csr_matrix((np.tile(np.array([0.25, -0.5, -0.5, 0.25]) * A1.val.max() / 64, n1),
                        (np.repeat(i, 4), ((i[:, None] + off[None, :]) % n1).ravel())), shape=(n1, n1))
    n_sys = n1
    g1 = np.arange(n_sys - 8, dtype=np.int32)
    cons = np.zeros(n_sys, dtype=bool)
    cons[n_sys - 8:] = True
    cons[:n_sys - 8] = lat1.boundary_mask()[:n_sys - 8]
    rng = np.random.default_rng(n_sys)
    empty = np.zeros(0, dtype=np.int32)
    return SimpleNamespace(system_matrix=A1, system_rhs=rng.standard_normal(n_sys) * ~cons, constrained=cons, level_matrices=[A0, A1],
                           edge_matrices=[None, _csr_ns(I1)], prolongations=[_csr_ns(P)], copy_global=[empty, g1], copy_level=[empty, g1.copy()])


@functools.lru_cache(maxsize=None)
def hierarchy(name):
    """(raw hierarchy, mg_reference.Hierarchy)"""
    if name == "hier3":
        h = so.build_uniform_hierarchy(3, 0.0, 1.0, 4, problem="Step16")
    elif name == "SYN":
        h = _synthetic()
    elif name == LAT:
        h = _lattice_case()
    elif name in REUSE_NAMES:
        h = _reuse_case(name)
    else:
        h = _adaptive(name)
    return h, R.Hierarchy(h, name)


# ------------------------------------------------------------------------------------------------ configurations

def given_bounds(n):
    """a caller-given partition with an empty block and a one-row block"""
    return (0, 70, 70, 71, n // 2 + 5, n)


def smoother_configs(name, level):
    n = hierarchy(name)[1].rows[level]
    C = R.Config
    out = [C(kind=R.JACOBI, steps=s) for s in (0, 1, 2, 3)]
    out += [C(kind=R.SSOR, steps=s, blocks=b) for s in (0, 1, 2, 3) for b in (1, 3)]
    out += [C(kind=R.SSOR, steps=s, blocks=5, bounds=((level, given_bounds(n)),)) for s in (1, 2, 3)]
    out += [C(kind=R.CHEBYSHEV, steps=s, degree=k, ratio=r) for s in (1, 2, 3) for k in (1, 2, 3, 4) for r in (30.0, 4.0)]
    out += [C(kind=R.CHEBYSHEV, steps=0, degree=3)]
    out += [C(kind=R.CHEBYSHEV, steps=s, degree=3, lmax=1.7) for s in (1, 2, 3)]
    return out


SSOR_VARIANTS = {"default": (), "sgs_reg": (("sgs_reg", 1),), "sgs_dep": (("sgs_dep", 1),), "sgs_disable_phase": (("sgs_disable_phase", 1),),
                 "sgs_disable_wave": (("sgs_disable_wave", 1),), "sgs_y_slots=300": (("sgs_y_slots", 300),)}

VCYCLE_CONFIGS = [R.Config(kind=k, steps=s, degree=2 + (s % 2)) for k in (R.JACOBI, R.SSOR, R.CHEBYSHEV) for s in (1, 2, 3)]
VCYCLE_CONFIGS.append(R.Config(kind=R.SSOR, steps=0))   # no smoothing at all: restrict, solve level 0, prolongate

# tests/test_gpu_ranks_reference.py: on N ranks the SSOR sweep is split among the ranks where N divides the
# number of blocks.  B = N and 2 N for N = 2, 3, a caller-given partition of N blocks with an empty block or a block of one row
# (tests/rank_cases.given_bounds), and the V-cycle with one block per rank.
RANK_BLOCKS = (2, 3, 4, 6)
RANK_SMOOTH_LEVELS = [("A3", 1), ("A3", 2), ("B3", 1), ("B3", 2)]
RANK_VCYCLE_CONFIGS = [R.Config(kind=R.SSOR, steps=s, degree=2 + (s % 2), blocks=b) for b in (2, 3) for s in (1, 2, 3)]


def rank_smoother_configs(name, level):
    import rank_cases as RC

    n = hierarchy(name)[1].rows[level]
    out = [R.Config(kind=R.SSOR, steps=s, blocks=b) for b in (1,) + RANK_BLOCKS for s in RC.MG_STEPS]
    for n_ranks in RC.MG_RANKS:
        out += [R.Config(kind=R.SSOR, steps=s, blocks=n_ranks, bounds=((level, bounds),)) for bounds in RC.given_bounds(n_ranks, n)
                for s in RC.MG_STEPS]
    return out


# bits of gmg_stats.spmv0_layout that a switch takes away from an operator that has them all (include/gmg_coulomb.h).  The
# lattice kernel needs the nine-run pattern and the value codes, not the pattern-run kernel: disable_sellp leaves it.
LAYOUT_CLEARS = {"disable_sell": 63, "disable_patterns": 8 + 16 + 32, "disable_compression": 2 + 4 + 8 + 16 + 32, "disable_sellp": 8 + 16,
                 "disable_rowclass": 16, "disable_lattice": 32}
LAYOUT_CFGS = [R.Config(kind=R.JACOBI, steps=3, degree=3), R.Config(kind=R.CHEBYSHEV, steps=2, degree=2)]                         # V-cycles on LAT
LAYOUT_SMOOTH = [R.Config(kind=R.JACOBI, steps=3), R.Config(kind=R.CHEBYSHEV, steps=2, degree=4), R.Config(kind=R.SSOR, steps=2)]   # smoother steps on LAT
LAYOUT_SWITCHES = ("disable_sell", "disable_patterns", "disable_compression", "disable_sellp", "disable_rowclass", "disable_lattice")


def smoother_vectors(name, level):
    n = hierarchy(name)[1].rows[level]
    rng = np.random.default_rng(1000 * level + n)
    return rng.standard_normal(n), rng.standard_normal(n)


def zero_rows(name):
    """global entries in no copy list (hanging nodes): the rows and columns of M that are exactly 0"""
    h, H = hierarchy(name)
    seen = np.zeros(H.n_sys, dtype=bool)
    for g in H.copy_global:
        seen[g] = True
    return np.flatnonzero(~seen)


def edge_dofs(name):
    """per level with an edge matrix, one global DoF that the edge terms of that level touch: a DoF on the refinement edge
    itself where the copy list holds one (a row of I_l), else a neighbour of the edge (a column of I_l; deal.II's copy lists
    leave the edge DoFs of a level to the coarser level)"""
    h, H = hierarchy(name)
    out = []
    for l in range(1, H.n_levels):
        I = H.I[l]
        if I is None:
            continue
        for busy in (np.flatnonzero(np.diff(I.indptr) > 0), np.unique(I.indices)):
            at = np.flatnonzero(np.isin(H.copy_level[l], busy))
            if len(at):
                out.append(int(H.copy_global[l][at[len(at) // 2]]))
                break
    return out


@functools.lru_cache(maxsize=None)
def vcycle_sources(name):
    """(src [n_sys, k], labels): random on all entries, random with the constrained entries zeroed (two of them: the pair of
    the symmetry check), unit vectors at a hanging node, at a refinement-edge DoF of each level, at a Dirichlet DoF and at the
    first and the last index.  dst0: what dst holds before the call."""
    h, H = hierarchy(name)
    n = H.n_sys
    rng = np.random.default_rng(n)
    free = ~np.asarray(h.constrained, dtype=bool)
    cols = [rng.standard_normal(n), rng.standard_normal(n) * free, rng.standard_normal(n) * free]
    labels = ["random", "random-free-x", "random-free-y"]
    zr = zero_rows(name)
    listed = np.setdiff1d(np.flatnonzero(~free), zr)   # constrained and in a copy list: Dirichlet (or a refinement edge)
    units = ([("hanging", int(zr[len(zr) // 2]))] if len(zr) else []) + [(f"edge{i}", d) for i, d in enumerate(edge_dofs(name))]
    units += ([("dirichlet", int(listed[0]))] if len(listed) else []) + [("first", 0), ("last", n - 1)]
    for lab, i in units:
        e = np.zeros(n)
        e[i] = 1.0
        cols.append(e)
        labels.append(lab)
    src = np.stack(cols, axis=1)
    src.setflags(write=False)
    dst0 = rng.standard_normal(n)
    dst0.setflags(write=False)
    return src, tuple(labels), dst0


# ------------------------------------------------------------------------------------------------ references (shared, cached)

@functools.lru_cache(maxsize=None)
def smoother_reference(name, level, cfg, from_zero):
    """namespace(ref [n] fp64 of the ld tier, S, tol): tolerance rule of mg_reference.tolerance, no coarse term"""
    H = hierarchy(name)[1]
    u0, rhs = smoother_vectors(name, level)
    f, l = (H.smooth(t, cfg, level, u0, rhs, from_zero) for t in R.TIERS)
    S = R.spread(f, l)
    ref = R.as_f64(l)
    ref.setflags(write=False)
    return SimpleNamespace(ref=ref, S=S, tol=float(R.tolerance(S, l)))


@functools.lru_cache(maxsize=None)
def vcycle_reference(name, cfg):
    """namespace(ref [n_sys, k] fp64 of the ld tier, S, tol [k] without the coarse allowance, coarse_norm [k], d0_norm [k])"""
    H = hierarchy(name)[1]
    src, labels, dst0 = vcycle_sources(name)
    seen = []

    def coarse(d):
        seen.append(R.norm2(d))
        return H.coarse_exact("ld", d)

    f = H.precondition("f64", cfg, src, dst0)
    l, cn = H.precondition("ld", cfg, src, dst0, coarse=coarse, want_coarse=True)
    S = R.spread(f, l)
    ref = R.as_f64(l)
    ref.setflags(write=False)
    return SimpleNamespace(ref=ref, S=S, tol=R.tolerance(S, l), coarse_norm=cn, d0_norm=seen[0], ld=l)


def level0_lattice(name):
    """(nv, Ke) of level 0 as gmg_set_level_matrix_lattice takes it, from the level-0 matrix alone: n = nv^3, and the cell
    size from the diagonal of an interior row of the Q1 Laplacian, 8 h / 3"""
    h, H = hierarchy(name)
    A0 = H.A[0]
    nv = int(round(A0.shape[0] ** (1.0 / 3.0)))
    assert nv ** 3 == A0.shape[0]
    centre = (nv // 2) * (1 + nv + nv * nv)
    cell = 3.0 * A0[centre, centre] / 8.0
    lat = so.Lattice(3, nv - 1, 0.0, cell)
    return (nv, nv, nv), np.array(so.cell_matrices(lat)[0]), lat
