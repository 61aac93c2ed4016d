"""The restatement of tests/refine_reference.py -- 2:1 closure and split, solution transfer, face table, written from the
definitions in include/gmg_coulomb.h -- against the host driver's Forest::refine_flagged,
LaplaceProblem::refine_grid and LaplaceProblem::face_table on the steps of tests/refine_cases.py, and what those steps contain.
Integer work and sums in a fixed order: every comparison is of equality, the transferred solution bit for bit."""
import numpy as np
import pytest

import mesh_tables_reference as mtr
import refine_cases as rc
import refine_reference as rr


@pytest.mark.parametrize("name", rc.STEPS)
def test_reference_equals_host(name):
    s = rc.step(name)
    rc.same_forest(s.ref.forest, s.new_fc, name)
    assert np.array_equal(np.asarray(s.ref.cell_parent, dtype=np.int32), s.parent), name
    assert np.array_equal(np.asarray(s.ref.closed_flag, dtype=np.uint8), s.closed), name
    assert s.ref.n_split == (len(s.new_fc.cell_first_child) - len(s.fc.cell_first_child)) >> s.fc.dim and s.ref.n_split > 0
    # the marks are on active cells, and the closure only adds
    assert not np.any(s.flag & (np.asarray(s.fc.cell_first_child) >= 0)) and np.all(s.closed >= s.flag)
    # the new numbering is the first-touch order of the new forest, and the transfer reproduces the host's bits
    assert np.array_equal(np.asarray(rr.active_vertices(s.new_fc), dtype=np.uint64), s.new_vertex), name
    assert np.array_equal(rc.bits(s.ref_u), rc.bits(s.u_new)), name
    for fc, (kind, cell) in ((s.fc, s.faces), (s.new_fc, s.new_faces)):
        k, c = rr.face_table(fc)
        assert np.array_equal(k, kind) and np.array_equal(c, cell), name


def test_the_host_steps_contain_the_cases():
    """all four face kinds; new vertices that are edge mid-points shared by several new cells, face centres and cell centres,
    every supplier with equal bits; constrained new DoFs that the transfer zeroes; a closure that adds flags"""
    kinds, shapes, zeroed, added = set(), set(), 0, 0
    for name in rc.STEPS:
        s = rc.step(name)
        kinds |= set(np.unique(s.new_faces[0]).tolist())
        added += int(np.sum(s.closed) - np.sum(s.flag))
        sup = {}
        u = rr.transfer(s.ref.forest, s.old_vertex, s.u_old, s.new_vertex, None, suppliers=sup)
        where = {int(k): i for i, k in enumerate(s.new_vertex)}
        for key, slots in sup.items():
            assert len({np.float64(v).view(np.uint64) for _, _, _, v in slots}) == 1, (name, key, slots)
            l, i, a, _ = slots[0]
            c = s.new_fc.cell_coord[s.new_fc.level_ptr[l] + i]
            odd = sum(int((c[d] + ((a >> d) & 1)) & 1) for d in range(s.fc.dim))   # directions in which the vertex is a mid-point
            shapes.add((s.fc.dim, odd, len(slots) > 1))
            if s.cons[where[key]] >= 0 and u[where[key]] != 0.0:
                zeroed += 1
                assert s.u_new[where[key]] == 0.0
    assert kinds == {0, 1, 2, 3}
    # 3D: edge mid-points (1) shared, face centres (2), cell centres (3); 2D: edge mid-points and cell centres (2)
    assert {(3, 1, True), (3, 2, True), (3, 3, True), (2, 1, True), (2, 2, True)} <= shapes, shapes
    assert zeroed > 0 and added > 0


@pytest.mark.parametrize("name", sorted(rc.HAND_BUILT))
def test_hand_built_steps(name):
    s = rc.hand(name)
    nch = 1 << s.fc.dim
    new = s.ref.forest
    assert len(new.cell_first_child) == len(s.fc.cell_first_child) + nch * s.ref.n_split
    mtr.build(new)   # balanced: no hanging vertex without a DoF
    rr.face_table(new)
    if name.startswith("single"):
        assert (s.fc.n_levels, new.n_levels, s.ref.n_split) == (1, 2, 1) and new.cell_first_child[0] == 0 and s.ref.cell_parent == [-1] + [0] * nch
        assert len(s.new_vertex) == 3 ** s.fc.dim and len([v for v in s.ref_u if v != 0.0]) == 1   # the centre alone is inside
    if name == "lattice-2x2":
        assert s.ref.closed_flag == [0, 1, 0, 0] and new.cell_first_child == [-1, 0, -1, -1, -1, -1, -1, -1]
        assert new.cell_coord[4:] == [[2, 0, 0], [3, 0, 0], [2, 1, 0], [3, 1, 0]] and s.ref.cell_parent[4:] == [1] * 4
    if name == "staircase-2d":
        lp = s.fc.level_ptr
        per_level = [sum(s.ref.closed_flag[lp[l]:lp[l + 1]]) - sum(s.flag[lp[l]:lp[l + 1]]) for l in range(3)]
        assert per_level == [5, 3, 0] and s.ref.n_split == 9   # (2, 0), (2, 1), (2, 2), (1, 2), (0, 2) on level 0
    if name in ("inactive-only", "no-flags", "zero-cells"):
        assert s.ref.n_split == 0 and not any(s.ref.closed_flag)
        rc.same_forest(new, s.fc, name)
        assert np.array_equal(rc.bits(s.ref_u), rc.bits([0.0 if c >= 0 else v for v, c in zip(s.u_old, s.cons)]))
    if name == "edge-3d":
        assert s.ref.n_split == 4   # the closure reaches the three level-0 neighbours of the refined cell


def test_reference_refusals():
    fc = rr.corner_12()
    assert fc.n_levels == 13
    with pytest.raises(rr.TooDeep):
        rr.refine(fc, rr.flags_at(fc, [(12, 0, 0, 0)]))
    assert rr.refine(fc, rr.flags_at(fc, [(11, 1, 1, 0)])).n_split >= 1   # level 11 may still be split
    hole = rr.hole_2d()
    with pytest.raises(rr.Unbalanced):
        rr.closure(hole, rr.flags_at(hole, [(1, 1, 0, 0)]))
    assert rr.refine(hole, rr.flags_at(hole, [(1, 0, 0, 0)])).n_split == 1   # (a flag away from the hole closes)
