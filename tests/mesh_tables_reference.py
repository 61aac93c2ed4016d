"""DoF numbering, constraint lines and level flags restated from the forest alone, in plain Python loops with dicts for the
maps: the definitions in the header comment of gmg_build_mesh_tables (include/gmg_coulomb.h), which restate the host's
LaplaceProblem::distribute_dofs and make_constraints (src/step-50.cc:661-706: dof_handler.distribute_dofs, distribute_mg_dofs,
make_hanging_node_constraints, interpolate_boundary_values, MGConstrainedDoFs).  Input: the namespace of
Problem.forest_cells() (or one built by forest() below).  Nothing here calls the library under test."""
from types import SimpleNamespace

SHIFT = 12


class Unbalanced(ValueError):
    """a hanging vertex without a DoF"""


def forest(dim, n0, levels, lexicographic):
    """namespace like Problem.forest_cells() from levels = [[(x, y, z, first_child), ...], ...]"""
    level_ptr, coord, fc = [0], [], []
    for cells in levels:
        for x, y, z, c in cells:
            coord.append([x, y, z])
            fc.append(c)
        level_ptr.append(len(fc))
    return SimpleNamespace(dim=dim, n0=list(n0), n_levels=len(levels), level_ptr=level_ptr, cell_coord=coord, cell_first_child=fc,
                           level0_lexicographic=bool(lexicographic))


def _lists(fc):
    as_list = lambda a: a.tolist() if hasattr(a, "tolist") else list(a)
    return as_list(fc.n0), as_list(fc.level_ptr), as_list(fc.cell_coord), as_list(fc.cell_first_child)


def pack(x, y, z):
    return x | (y << 21) | (z << 42)


def vertex_key(dim, level, c, v):
    s = SHIFT - level
    return pack((c[0] + (v & 1)) << s, (c[1] + ((v >> 1) & 1)) << s, (c[2] + ((v >> 2) & 1)) << s if dim == 3 else 0)


def unpack(key):
    return [key & 0x1FFFFF, (key >> 21) & 0x1FFFFF, (key >> 42) & 0x1FFFFF]


def on_boundary(dim, n0, key):
    v = unpack(key)
    for d in range(dim):
        if v[d] == 0 or v[d] == n0[d] << SHIFT:
            return True
    return False


def first_touch(dim, cells):
    """cells: [(level, coord)] in visiting order -> (cell_dofs, vertex_of_dof, dof_of_vertex)"""
    dof_of, vertex_of, table = {}, [], []
    for level, c in cells:
        row = []
        for v in range(1 << dim):
            key = vertex_key(dim, level, c, v)
            if key not in dof_of:
                dof_of[key] = len(vertex_of)
                vertex_of.append(key)
            row.append(dof_of[key])
        table.append(row)
    return table, vertex_of, dof_of


def build(fc):
    """namespace(n_cells, n_dofs, n_hanging, n_lines, cell_dofs, cell_level, vertex_of_dof, constraint_of_dof, line_ptr,
    line_master, line_weight, line_dof, levels = [namespace(n_cells, n_dofs, cell_dofs, vertex_of_dof, dof_flags)], n_visits:
    how often a qualifying face reached a hanging vertex); the lines are unclosed.  Raises Unbalanced."""
    dim = fc.dim
    nv, n_levels = 1 << dim, fc.n_levels
    n0, level_ptr, coord, first_child = _lists(fc)
    if dim == 2:
        n0 = [n0[0], n0[1], 1]
    cell_of = [{} for _ in range(n_levels)]   # per level: coordinates -> index within the level
    for l in range(n_levels):
        for c in range(level_ptr[l], level_ptr[l + 1]):
            cell_of[l][tuple(coord[c])] = c - level_ptr[l]
    # active cells by (level, index)
    active = [(l, c) for l in range(n_levels) for c in range(level_ptr[l], level_ptr[l + 1]) if first_child[c] < 0]
    cell_dofs, vertex_of_dof, dof_of = first_touch(dim, [(l, coord[c]) for l, c in active])
    n_dofs = len(vertex_of_dof)
    # levels
    levels = []
    for l in range(n_levels):
        cells = [(l, coord[c]) for c in range(level_ptr[l], level_ptr[l + 1])]
        if l == 0 and fc.level0_lexicographic and level_ptr[n_levels] > 0:
            nx, ny, nz = n0[0] + 1, n0[1] + 1, (n0[2] + 1 if dim == 3 else 1)
            assert len(cells) == n0[0] * n0[1] * n0[2], "level 0 is not the full lattice"
            for i, (_, c) in enumerate(cells):
                assert c == [i % n0[0], (i // n0[0]) % n0[1], i // (n0[0] * n0[1])], "level 0 is not in lexicographic order"
            vert = [pack(i << SHIFT, j << SHIFT, k << SHIFT) for k in range(nz) for j in range(ny) for i in range(nx)]
            table = [[(c[0] + (v & 1)) + nx * ((c[1] + ((v >> 1) & 1)) + ny * ((c[2] + ((v >> 2) & 1)) if dim == 3 else 0)) for v in range(nv)]
                     for _, c in cells]
        else:
            table, vert, _ = first_touch(dim, cells)
        flags = [1 if on_boundary(dim, n0, key) else 0 for key in vert]
        if l >= 1:
            for i, (_, c) in enumerate(cells):
                for d in range(dim):
                    for side in (0, 1):
                        nb = list(c)
                        nb[d] += 1 if side else -1
                        if nb[d] < 0 or nb[d] >= n0[d] << l or tuple(nb) in cell_of[l]:
                            continue
                        for v in range(nv):
                            if (v >> d) & 1 == side:
                                flags[table[i][v]] |= 2
        levels.append(SimpleNamespace(n_cells=len(cells), n_dofs=len(vert), cell_dofs=table, vertex_of_dof=vert, dof_flags=flags))
    # hanging-node lines
    constraint_of_dof = [-1] * n_dofs
    line_dof, line_ptr, line_master, line_weight = [], [0], [], []
    visits = [(0, 1, 2, 3), (0, 1), (2, 3), (0, 2), (1, 3)] if dim == 3 else [(0, 1)]
    n_visits = 0
    for a, (l, c) in enumerate(active):
        for d in range(dim):
            for side in (0, 1):
                nb = list(coord[c])
                nb[d] += 1 if side else -1
                N = cell_of[l].get(tuple(nb))
                if N is None or first_child[level_ptr[l] + N] < 0:
                    continue
                on_face = [v for v in range(nv) if (v >> d) & 1 == side]
                corner = [unpack(vertex_key(dim, l, coord[c], v)) for v in on_face]
                for ids in visits:
                    m = len(ids)
                    s = [0, 0, 0]
                    for q in ids:
                        for e in range(3):
                            s[e] += corner[q][e]
                    key = pack(s[0] // m, s[1] // m, s[2] // m)
                    if key not in dof_of:
                        raise Unbalanced("hanging node without a DoF: the mesh is not 2:1 balanced")
                    dof = dof_of[key]
                    n_visits += 1
                    if constraint_of_dof[dof] >= 0:
                        continue
                    constraint_of_dof[dof] = len(line_dof)
                    line_dof.append(dof)
                    for q in ids:
                        line_master.append(cell_dofs[a][on_face[q]])
                        line_weight.append(1.0 / m)
                    line_ptr.append(len(line_master))
    n_hanging = len(line_dof)
    # Dirichlet lines
    for i in range(n_dofs):
        if on_boundary(dim, n0, vertex_of_dof[i]) and constraint_of_dof[i] < 0:
            constraint_of_dof[i] = len(line_dof)
            line_dof.append(i)
            line_ptr.append(len(line_master))
    return SimpleNamespace(n_cells=len(active), n_dofs=n_dofs, n_hanging=n_hanging, n_lines=len(line_dof), cell_dofs=cell_dofs,
                           cell_level=[l for l, _ in active], vertex_of_dof=vertex_of_dof, constraint_of_dof=constraint_of_dof, line_ptr=line_ptr,
                           line_master=line_master, line_weight=line_weight, line_dof=line_dof, levels=levels, n_visits=n_visits)


def close(r, dirichlet_value):
    """constraints.close() on the unclosed lines of build(): dirichlet_value[k] is the inhomogeneity of Dirichlet line
    n_hanging + k.  A master that carries a Dirichlet line folds into the inhomogeneity (entries in stored order, from 0.0) and
    is dropped.  Returns (line_ptr, line_master, line_weight, line_inhomogeneity)."""
    inhom = [0.0] * r.n_hanging + [float(v) for v in dirichlet_value]
    assert len(inhom) == r.n_lines
    ptr, master, weight = [0], [], []
    for l in range(r.n_lines):
        for e in range(r.line_ptr[l], r.line_ptr[l + 1]):
            cm = r.constraint_of_dof[r.line_master[e]]
            if cm < 0:
                master.append(r.line_master[e])
                weight.append(r.line_weight[e])
                continue
            assert cm >= r.n_hanging, "hanging node constrained to a hanging node"
            inhom[l] += r.line_weight[e] * inhom[cm]
        ptr.append(len(master))
    return ptr, master, weight, inhom


# ------------------------------------------------------------------------------------------------ hand-built forests

def _children(x, y, z, dim):
    return [(2 * x + (a & 1), 2 * y + ((a >> 1) & 1), 2 * z + ((a >> 2) & 1) if dim == 3 else 0, -1) for a in range(1 << dim)]


def single_cell(dim, lexicographic=True):
    return forest(dim, (1, 1, 1), [[(0, 0, 0, -1)]], lexicographic)


def empty(dim):
    return forest(dim, (1, 1, 1), [[]], True)


def quadrant_2d(lexicographic=True):
    """a 2 x 2 lattice with cell 0 refined: two hanging nodes, one reached from cell 1 and one from cell 2"""
    return forest(2, (2, 2, 1), [[(0, 0, 0, 0), (1, 0, 0, -1), (0, 1, 0, -1), (1, 1, 0, -1)], _children(0, 0, 0, 2)], lexicographic)


def edge_only_3d(lexicographic=True):
    """a 2 x 2 x 1 lattice with cell 0 refined: cell 3 touches it across the edge x = y = 1 only; the mid-point of that edge
    hangs on the faces of cells 1 and 2 (visited twice, one line), and cell 3 holds both of its masters"""
    return forest(3, (2, 2, 1), [[(0, 0, 0, 0), (1, 0, 0, -1), (0, 1, 0, -1), (1, 1, 0, -1)], _children(0, 0, 0, 3)], lexicographic)


def unbalanced_2d():
    """a 3 x 1 lattice whose cell 0 claims the children that lie inside cell 2: the mid-point of the face between cells 0 and 1
    hangs without a DoF"""
    return forest(2, (3, 1, 1), [[(0, 0, 0, 0), (1, 0, 0, -1), (2, 0, 0, -1)], _children(2, 0, 0, 2)], False)
