"""The two-level meshes that tests/test_transfer_reference_cpu.py and tests/test_gpu_transfer_reference.py share (DESIGN.md
section 31): each the smallest at which one edge of gmg_build_transfer exists.  A case is generated from a coarse cell lattice,
the subset of its cells that is refined, an origin offset in lattice units, fine_spacing, boundary flags (geometric: the
lattice's faces; or drawn) and a numbering seed; both levels are numbered by a seeded random permutation unless the case is
one of the driver's meshes.  Vertex keys are x | y << 21 | z << 42 as include/gmg_coulomb.h packs them.  Computed once, left
unchanged; the sizes are asserted, so a drifting case fails instead of silently shrinking."""
import functools
from types import SimpleNamespace

import numpy as np

import transfer_reference as TR

DENSE_LIMIT = 2000   # evaluator A (quadratic) runs on the cases with at most this many fine rows
TOP = 1 << 21

#  name: (coarse DoFs, fine DoFs, nnz of P) as generated
SIZES = {
    "one-cell-2d": (4, 9, 0), "one-cell-3d": (8, 27, 0), "centre-3d": (27, 125, 27),
    "L-3d": (343, 1333, 1975), "L-3d-drawn": (343, 1333, 2785), "checker-2d": (100, 222, 319), "two-cells-3d": (125, 54, 64),
    "top-L-3d": (343, 1333, 1975), "top-checker-2d": (100, 222, 319), "origin-L-3d": (343, 1333, 1975), "origin-checker-2d": (100, 222, 319),
    "origin-L-3d-drawn": (343, 1333, 2914),
    "spacing-1": (343, 1333, 1975), "spacing-4096": (343, 1333, 1975), "spacing-2p18": (64, 183, 88),
    "load-512": (512, 31 * 63, 3780), "load-513": (513, 37 * 53, 3825),
    "scan-c16384": (16384, 255 * 255, 142884), "scan-c16385": (16385, 225 * 289, 142857),
    "scan-f16384": (65 * 68, 125 * 131 + 9, 35894), "scan-f16385": (57 * 73, 16385, 35145), "scan-f32769": (5 * 1821, 32769, 49113),
    "mesh-A3-0": (729, 1303, 2708), "mesh-A3-1": (1303, 250, 686), "mesh-S2": (237, 18, 32),
}
NAMES = tuple(SIZES)
MESH = {"mesh-A3-0": ("A3", 0), "mesh-A3-1": ("A3", 1), "mesh-S2": ("S2-c2", -1)}   # (case of mesh_tables_cases, coarse level; -1: the finest transfer)
TOP_OF_RANGE = ("top-L-3d", "top-checker-2d")
SCAN = ("scan-c16384", "scan-c16385", "scan-f16384", "scan-f16385", "scan-f32769")


def _l_shape(n):
    """c0 in the upper half, or c1 and c2 both in the lowest third: c0 >= 3 or (c1 < 2 and c2 < 2) on 6^3 cells"""
    return lambda c: (2 * c[0] >= n) | ((3 * c[1] < n) & (3 * c[2] < n))


def _lattice(name, dim, n_cells, refined, offset, fine_spacing, flags="geometric", seed=0):
    """refined: function of the cell index arrays (c0, c1[, c2]) -> mask"""
    h, H = int(fine_spacing), 2 * int(fine_spacing)
    n = list(n_cells) + [0] * (3 - dim)
    off = np.array(list(offset) + [0] * (3 - dim), dtype=np.int64)
    rng = np.random.default_rng(seed)
    # coarse level: every vertex of the lattice, x fastest, then permuted
    idx = np.stack(np.meshgrid(*[np.arange(m + 1) for m in n], indexing="ij"), axis=-1).reshape(-1, 3)
    idx = idx[np.lexsort((idx[:, 0], idx[:, 1], idx[:, 2]))]
    if flags == "geometric":
        boundary = np.zeros(len(idx), dtype=bool)
        for d in range(dim):
            boundary |= (idx[:, d] == 0) | (idx[:, d] == n[d])
    else:
        boundary = rng.random(len(idx)) < float(flags)
    perm = rng.permutation(len(idx))
    coarse_xyz = ((idx + off) * H)[perm]
    coarse_boundary = boundary[perm].astype(np.uint8)
    # refined cells and the fine level: the 3^dim vertices of the children of every refined cell
    cidx = np.stack(np.meshgrid(*[np.arange(max(m, 1)) for m in n], indexing="ij"), axis=-1).reshape(-1, 3)
    cidx = cidx[refined([cidx[:, d] for d in range(dim)])]
    cells = (cidx + off) * H
    t = np.stack(np.meshgrid(*[np.arange(3) if d < dim else np.arange(1) for d in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
    fine_xyz = np.unique((cells[:, None, :] + h * t[None, :, :]).reshape(-1, 3), axis=0)
    fine_xyz = fine_xyz[rng.permutation(len(fine_xyz))]
    assert coarse_xyz.min() >= 0 and max(coarse_xyz.max(), fine_xyz.max()) < TOP, name
    key = lambda v: (v[:, 0].astype(np.uint64) | (v[:, 1].astype(np.uint64) << np.uint64(21)) | (v[:, 2].astype(np.uint64) << np.uint64(42)))
    return _finish(name, dim, key(coarse_xyz), coarse_boundary, key(fine_xyz), cells, h, random_numbering=True)


def _finish(name, dim, coarse_vertex, coarse_boundary, fine_vertex, cells, fine_spacing, random_numbering, host_P=None):
    P, Pt = TR.from_cells(dim, coarse_vertex, coarse_boundary, fine_vertex, cells, fine_spacing)
    dense = TR.from_vertices(dim, coarse_vertex, coarse_boundary, fine_vertex, fine_spacing) if len(fine_vertex) <= DENSE_LIMIT else None
    want = SIZES[name]
    got = (len(coarse_vertex), len(fine_vertex), P.nnz)
    assert all(w is None or w == g for w, g in zip(want, got)), (name, got, want)   # a drifting case must fail
    for a in (coarse_vertex, coarse_boundary, fine_vertex, cells, P.rowptr, P.col, P.val, Pt.rowptr, Pt.col, Pt.val):
        a.setflags(write=False)
    return SimpleNamespace(name=name, dim=dim, coarse_vertex=coarse_vertex, coarse_boundary=coarse_boundary, fine_vertex=fine_vertex, cells=cells,
                           fine_spacing=int(fine_spacing), P=P, Pt=Pt, dense=dense, random_numbering=random_numbering, host_P=host_P,
                           n_coarse=len(coarse_vertex), n_fine=len(fine_vertex))


def _top(n_cells, H):
    """the offset that puts the lattice's largest coordinate on the largest multiple of H below 2^21"""
    return [TOP // H - 1 - m for m in n_cells]


def _mesh(name):
    """one transfer of a mesh of the driver: vertex_of_dof and dof_flags bit 0 of the numpy restatement of the mesh tables,
    the forest's refined cells, fine_spacing = 1 << (12 - fine level); host_P: the host-built P of the same level"""
    import mesh_tables_cases as MC
    import mg_cases

    which, level = MESH[name]
    snap = MC.case(which)
    fc, ref = snap.fc, snap.ref
    if level < 0:
        level = fc.n_levels - 2
    if which == "A3":
        host = mg_cases.hierarchy("A3")[0].prolongations[level]
    else:
        host = _s2_prolongations()[level]
    lp = np.asarray(fc.level_ptr, dtype=np.int64)
    coord = np.asarray(fc.cell_coord, dtype=np.int64).reshape(-1, 3)[lp[level]:lp[level + 1]]
    first_child = np.asarray(fc.cell_first_child, dtype=np.int64)[lp[level]:lp[level + 1]]
    cells = coord[first_child >= 0] << (12 - level)
    if fc.dim == 2:
        cells[:, 2] = 0
    lv, fv = ref.levels[level], ref.levels[level + 1]
    return _finish(name, fc.dim, np.array(lv.vertex_of_dof, dtype=np.uint64), (np.array(lv.dof_flags, dtype=np.uint8) & 1).astype(np.uint8),
                   np.array(fv.vertex_of_dof, dtype=np.uint64), cells, 1 << (12 - (level + 1)), random_numbering=False, host_P=host)


@functools.lru_cache(maxsize=None)
def _s2_prolongations():
    """the host-built prolongations of mesh_tables_cases.case("S2-c2"): the same run (mesh_tables_cases._cycles keeps the
    forest, not the hierarchy)"""
    import mesh_tables_cases as MC
    from oracle import gmg_oracle as go

    family, last = MC.CASES["S2-c2"]
    p, smoother, _ = MC._open(family)
    for cycle in range(last + 1):
        p.run_cycle(cycle, on_device=False)
        h = p.hierarchy()
        if cycle < last:
            p.finish_cycle_with(go.OracleMG(h, smoother=getattr(go, smoother)).solve(h.system_rhs, x0=p.vector("initial_guess"))["x"])
    p.close()
    return h.prolongations


@functools.lru_cache(maxsize=None)
def case(name):
    every = lambda c: np.ones(len(c[0]), dtype=bool)
    checker = lambda c: (c[0] + c[1]) % 3 == 0
    L6 = dict(dim=3, n_cells=(6, 6, 6), refined=_l_shape(6))
    C9 = dict(dim=2, n_cells=(9, 9), refined=checker)
    fs = 8   # where a case does not set it
    if name in MESH:
        return _mesh(name)
    if name == "one-cell-2d":
        return _lattice(name, 2, (1, 1), every, (3, 5), fs, seed=1)
    if name == "one-cell-3d":
        return _lattice(name, 3, (1, 1, 1), every, (3, 5, 2), fs, seed=2)
    if name == "centre-3d":
        return _lattice(name, 3, (2, 2, 2), every, (1, 4, 2), fs, seed=3)
    if name == "L-3d":
        return _lattice(name, offset=(2, 1, 3), fine_spacing=fs, seed=4, **L6)
    if name == "L-3d-drawn":
        return _lattice(name, offset=(2, 1, 3), fine_spacing=fs, flags=0.3, seed=5, **L6)
    if name == "checker-2d":
        return _lattice(name, offset=(4, 1), fine_spacing=fs, seed=6, **C9)
    if name == "two-cells-3d":
        return _lattice(name, 3, (4, 4, 4), lambda c: ((c[0] == 1) & (c[1] == 2) & (c[2] == 3)) | ((c[0] == 2) & (c[1] == 1) & (c[2] == 0)), (1, 1, 1), fs, seed=7)
    if name == "top-L-3d":
        return _lattice(name, offset=_top((6, 6, 6), 2 * fs), fine_spacing=fs, seed=8, **L6)
    if name == "top-checker-2d":
        return _lattice(name, offset=_top((9, 9), 2 * fs), fine_spacing=fs, seed=9, **C9)
    if name == "origin-L-3d":
        return _lattice(name, offset=(0, 0, 0), fine_spacing=fs, seed=10, **L6)
    if name == "origin-checker-2d":
        return _lattice(name, offset=(0, 0), fine_spacing=fs, seed=11, **C9)
    if name == "origin-L-3d-drawn":   # interior coarse DoFs at coordinate 0: with geometric flags the rows there are empty
        return _lattice(name, offset=(0, 0, 0), fine_spacing=fs, flags=0.3, seed=22, **L6)
    if name == "spacing-1":
        return _lattice(name, offset=(2, 1, 3), fine_spacing=1, seed=12, **L6)
    if name == "spacing-4096":
        return _lattice(name, offset=(2, 1, 3), fine_spacing=4096, seed=13, **L6)
    if name == "spacing-2p18":   # H = 2^19: four coarse vertices per direction are all the key admits
        return _lattice(name, 3, (3, 3, 3), _l_shape(3), (0, 0, 0), 1 << 18, seed=14)
    if name == "load-512":
        return _lattice(name, 2, (15, 31), every, (1, 2), fs, seed=15)
    if name == "load-513":
        return _lattice(name, 2, (18, 26), every, (1, 2), fs, seed=16)
    if name == "scan-c16384":
        return _lattice(name, 2, (127, 127), every, (1, 2), fs, seed=17)
    if name == "scan-c16385":
        return _lattice(name, 2, (112, 144), every, (1, 2), fs, seed=18)
    if name == "scan-f16384":   # 125 * 131 + 9 fine vertices
        return _lattice(name, 2, (64, 67), lambda c: ((c[0] < 62) & (c[1] < 65)) | ((c[0] == 63) & (c[1] == 66)), (1, 2), fs, seed=19)
    if name == "scan-f16385":
        return _lattice(name, 2, (56, 72), every, (1, 2), fs, seed=20)
    if name == "scan-f32769":
        return _lattice(name, 2, (4, 1820), every, (1, 2), fs, seed=21)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def vectors(name):
    """(x [n_coarse], r [n_fine], dst0 [n_coarse]): magnitudes over six decades, every sign; dst0 nowhere zero"""
    c = case(name)
    rng = np.random.default_rng(c.n_coarse + 7 * c.n_fine)
    draw = lambda n: rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * 10.0 ** rng.permutation(np.linspace(-3.0, 3.0, n))
    out = draw(c.n_coarse), draw(c.n_fine), draw(c.n_coarse)
    for a in out:
        a.setflags(write=False)
    return out
