"""The step between two cycles restated from the definitions in include/gmg_coulomb.h alone (gmg_refine_forest,
gmg_transfer_solution, gmg_build_face_table): the 2:1 closure of the marks as a literal least fixed point,
the split, the solution transfer as the stated sum in Python floats, and the estimator's face table from a brute-force search
over the boxes of the active cells (as tests/kelly_reference.py finds its neighbours: no tree is walked, no cell is looked up by
its coordinates).  Plain Python with dicts and sets.  Input: the namespace of Problem.forest_cells() or one built by
mesh_tables_reference.forest().  Nothing here calls the library under test."""
from types import SimpleNamespace

import numpy as np

from mesh_tables_reference import _lists, pack, vertex_key

MAX_LEVEL = 12


class Unbalanced(ValueError):
    """a neighbour position with no cell on the level and none on the level below / a face that is not 2:1 balanced"""


class TooDeep(ValueError):
    """a split on level 12"""


class NoValue(ValueError):
    """a parent vertex without an old value"""


def levels_of(fc):
    """[[(x, y, z, first_child), ...] per level]"""
    _, level_ptr, coord, first_child = _lists(fc)
    return [[tuple(coord[c]) + (first_child[c],) for c in range(level_ptr[l], level_ptr[l + 1])] for l in range(fc.n_levels)]


def closure(fc, flag):
    """the closed flags, [[0 / 1 per cell] per level]: the least fixed point, iterated until nothing changes"""
    dim = fc.dim
    n0 = list(fc.n0)[:dim] + [1] * (3 - dim)
    lv = levels_of(fc)
    _, level_ptr, _, _ = _lists(fc)
    flag = [int(v) for v in flag]
    F = [[1 if flag[level_ptr[l] + i] and c[3] < 0 else 0 for i, c in enumerate(cells)] for l, cells in enumerate(lv)]
    cell_of = [{c[:3]: i for i, c in enumerate(cells)} for cells in lv]
    changed = True
    while changed:
        changed = False
        for l in range(1, len(lv)):
            for i, c in enumerate(lv[l]):
                if not F[l][i] or c[3] >= 0:
                    continue
                for dz in ((-1, 0, 1) if dim == 3 else (0,)):
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            p = (c[0] + dx, c[1] + dy, c[2] + dz)
                            if p == c[:3] or any(p[e] < 0 or p[e] >= n0[e] << l for e in range(dim)):
                                continue
                            if p in cell_of[l]:
                                continue
                            q = cell_of[l - 1].get((p[0] >> 1, p[1] >> 1, p[2] >> 1))
                            if q is None:
                                raise Unbalanced("the forest is not vertex-balanced")
                            if not F[l - 1][q]:
                                F[l - 1][q] = 1
                                changed = True
    return F


def refine(fc, flag):
    """namespace(forest: the new forest like Problem.forest_cells(), cell_parent, closed_flag, n_split)"""
    dim, nch = fc.dim, 1 << fc.dim
    lv = levels_of(fc)
    F = closure(fc, flag)
    if lv and any(F[-1]) and len(lv) - 1 >= MAX_LEVEL:
        raise TooDeep("a split on level 12")
    new = [[list(c) for c in cells] for cells in lv]
    if lv and any(F[-1]):
        new.append([])
    parent = [[-1] * len(cells) for cells in new]
    for l in range(1, len(lv)):
        where = {c[:3]: i for i, c in enumerate(lv[l - 1])}
        parent[l] = [where[(c[0] >> 1, c[1] >> 1, c[2] >> 1)] for c in lv[l]]
    n_split = 0
    for l in range(len(lv)):                     # the levels independently: the children go behind the old cells of level l + 1
        old_size, rank = (len(lv[l + 1]) if l + 1 < len(lv) else 0), 0
        for i, c in enumerate(lv[l]):
            if not F[l][i]:
                continue
            new[l][i][3] = old_size + nch * rank
            for a in range(nch):
                new[l + 1].append([2 * c[0] + (a & 1), 2 * c[1] + ((a >> 1) & 1), 2 * c[2] + ((a >> 2) & 1) if dim == 3 else 0, -1])
                parent[l + 1].append(i)
            rank += 1
        n_split += rank
    level_ptr, coord, first_child = [0], [], []
    for cells in new:
        coord += [c[:3] for c in cells]
        first_child += [c[3] for c in cells]
        level_ptr.append(len(first_child))
    forest = SimpleNamespace(dim=dim, n0=list(fc.n0), n_levels=len(new), level_ptr=level_ptr, cell_coord=coord, cell_first_child=first_child,
                             level0_lexicographic=getattr(fc, "level0_lexicographic", True))
    return SimpleNamespace(forest=forest, cell_parent=[p for lvl in parent for p in lvl], closed_flag=[f for lvl in F for f in lvl], n_split=n_split)


def weights(dim, child, a):
    """w_p of vertex a of the child: products in ascending d"""
    out = []
    for p in range(1 << dim):
        w = 1.0
        for d in range(dim):
            pos = 0.5 * (((child >> d) & 1) + ((a >> d) & 1))
            w *= pos if (p >> d) & 1 else 1.0 - pos
        out.append(w)
    return out


def transfer(new_fc, old_vertex_of_dof, u_old, new_vertex_of_dof, constraint_of_dof=None, suppliers=None):
    """u_new as a list of Python floats.  suppliers (a dict, optional) collects per new vertex key the list of (level, cell,
    vertex, value) of EVERY slot that can supply it -- the value returned is the first one's, as on the host."""
    dim, nv = new_fc.dim, 1 << new_fc.dim
    old = {int(k): float(v) for k, v in zip(old_vertex_of_dof, u_old)}
    value = dict(old)
    lv = levels_of(new_fc)
    for l in range(1, len(lv)):
        for i, c in enumerate(lv[l]):
            child = (c[0] & 1) | ((c[1] & 1) << 1) | (((c[2] & 1) << 2) if dim == 3 else 0)
            pc = (c[0] >> 1, c[1] >> 1, c[2] >> 1)
            for a in range(nv):
                key = vertex_key(dim, l, c, a)
                if key in old:
                    continue
                w = weights(dim, child, a)
                v = 0.0
                for p in range(nv):
                    pk = vertex_key(dim, l - 1, pc, p)
                    if pk not in old:
                        raise NoValue("a parent vertex without an old value")
                    v += w[p] * old[pk]
                if suppliers is not None:
                    suppliers.setdefault(key, []).append((l, i, a, v))
                value.setdefault(key, v)
    out = [value[int(k)] for k in new_vertex_of_dof]
    if constraint_of_dof is not None:
        out = [0.0 if c >= 0 else v for v, c in zip(out, constraint_of_dof)]
    return out


def face_table(fc):
    """(face_kind [n_active, 2 dim], face_cell [n_active, 2 dim, 2^(dim-1)]) by a search over the boxes of the active cells"""
    dim = fc.dim
    nfc, nf = 1 << (dim - 1), 2 * dim
    lv = levels_of(fc)
    act = [(l, c) for l, cells in enumerate(lv) for c in cells if c[3] < 0]
    n = len(act)
    fk, fcell = np.zeros((n, nf), dtype=np.uint8), np.zeros((n, nf, nfc), dtype=np.int32)
    if n == 0:
        return fk, fcell
    L = max(l for l, _ in act)
    level = np.array([l for l, _ in act], dtype=np.int64)
    size = 1 << (L - level)
    lo = np.array([c[:dim] for _, c in act], dtype=np.int64) * size[:, None]
    inface = [[e for e in range(dim) if e != d] for d in range(dim)]
    for a in range(n):
        for d in range(dim):
            for side in (0, 1):
                plane = lo[a, d] + size[a] if side else lo[a, d]
                m = (lo[:, d] == plane) if side else (lo[:, d] + size == plane)
                for e in inface[d]:
                    m &= (lo[:, e] < lo[a, e] + size[a]) & (lo[:, e] + size > lo[a, e])
                nb = np.nonzero(m)[0]
                f = 2 * d + side
                if len(nb) == 0:
                    continue
                if len(nb) == 1 and level[nb[0]] == level[a]:
                    fk[a, f], fcell[a, f, 0] = 1, nb[0]
                elif len(nb) == 1 and level[nb[0]] == level[a] - 1:
                    b = nb[0]
                    quad = sum(int((lo[a, e] - lo[b, e]) // size[a]) << k for k, e in enumerate(inface[d]))
                    fk[a, f], fcell[a, f, 0], fcell[a, f, 1] = 3, b, quad
                elif len(nb) == nfc and all(level[b] == level[a] + 1 for b in nb):
                    fk[a, f] = 2
                    for b in nb:
                        quad = sum(int((lo[b, e] - lo[a, e]) // size[b]) << k for k, e in enumerate(inface[d]))
                        fcell[a, f, quad] = b
                else:
                    raise Unbalanced("mesh not 2:1 balanced across a face")
    return fk, fcell


def active_vertices(fc):
    """the vertex keys of the active mesh in first-touch order (the numbering of gmg_build_mesh_tables)"""
    seen, out = set(), []
    for l, cells in enumerate(levels_of(fc)):
        for c in cells:
            if c[3] >= 0:
                continue
            for v in range(1 << fc.dim):
                k = vertex_key(fc.dim, l, c, v)
                if k not in seen:
                    seen.add(k)
                    out.append(k)
    return out


# ------------------------------------------------------------------------------------------------ hand-built forests

def lattice(dim, n):
    from mesh_tables_reference import forest
    nz = n if dim == 3 else 1
    return forest(dim, (n, n, nz), [[(i, j, k, -1) for k in range(nz) for j in range(n) for i in range(n)]], True)


def flags_at(fc, where):
    """a flag array with the cells (level, x, y, z) flagged"""
    lv = levels_of(fc)
    _, level_ptr, _, _ = _lists(fc)
    flag = [0] * level_ptr[-1]
    for l, x, y, z in where:
        flag[level_ptr[l] + [c[:3] for c in lv[l]].index((x, y, z))] = 1
    return flag


def refined(fc, *rounds):
    """the forest after refining the cells of each round in turn: vertex-balanced by construction"""
    for where in rounds:
        fc = refine(fc, flags_at(fc, where)).forest
    return fc


def staircase_2d():
    """a 4 x 4 lattice refined at (0, 0), then at the level-1 cells (1, 1) and (2, 2): level 1 covers [0, 4)^2 and level 2 holds
    the cells (2..3)^2 and (4..5)^2.  A flag on the level-2 cell (5, 5) forces the level-1 cells (3, 2), (2, 3), (3, 3), and
    these in turn force the level-0 cells (2, 0), (2, 1), (2, 2), (1, 2), (0, 2)"""
    return refined(lattice(2, 4), [(0, 0, 0, 0)], [(1, 1, 1, 0)], [(1, 2, 2, 0)])


def hole_2d():
    """a 2 x 1 lattice that lacks its cell (1, 0) while cell (0, 0) is refined: the level-1 cell (1, 0) has no neighbour at
    (2, 0) and none on the level below -- not vertex-balanced"""
    from mesh_tables_reference import _children, forest
    return forest(2, (2, 1, 1), [[(0, 0, 0, 0)], _children(0, 0, 0, 2)], False)


def corner_12():
    """a single 2D cell refined 12 times towards its corner (0, 0): the finest cell is on level 12"""
    fc = lattice(2, 1)
    for l in range(MAX_LEVEL):
        fc = refine(fc, flags_at(fc, [(l, 0, 0, 0)])).forest
    return fc
