"""The refinement steps that tests/test_refine_cpu.py and tests/test_gpu_refine.py share: consecutive cycles of the families of
tests/mesh_tables_cases.py, driven on the host with the host's own marks and the oracle's solutions (or, "-rnd", a random vector
in the solution's place), and hand-built forests.  Per step: the forest and the marks that went in, the old solution by vertex,
the host's new forest, closed marks, transferred solution and face table, and the restatement of tests/refine_reference.py --
computed once, left unchanged."""
import functools
from types import SimpleNamespace

import numpy as np

import mesh_tables_cases as mtc
import mesh_tables_reference as mtr
import refine_reference as rr

#  family: last cycle.  "-rnd": one step whose old solution is random (distributed: hanging and boundary values as the lines say)
FAMILIES = {"A3": 3, "B3": 3, "G8": 2, "S2": 2, "S3": 1, "CW": 1, "G8-rnd": 1, "S2-rnd": 1}
STEPS = [f"{f}:{c}->{c + 1}" for f, last in FAMILIES.items() for c in range(last)]


def _face_table(p):
    e = p.estimator_inputs()
    return e.face_kind, e.face_cell


@functools.lru_cache(maxsize=None)
def _family(family):
    from oracle import gmg_oracle as go

    last = FAMILIES[family]
    p, smoother, _ = mtc._open(family.split("-")[0])
    rng = np.random.default_rng(50)
    steps, before = [], None
    for cycle in range(last + 1):
        p.run_cycle(cycle, on_device=False)
        fc = p.forest_cells()
        faces = _face_table(p)
        if before is not None:
            s = before
            s.new_fc, s.parent, s.closed, s.new_vertex = fc, p.forest_parents(), p.closed_flags(), p.vertex_keys()
            s.cons, s.u_new, s.new_faces = p.system_assembly_inputs().constraint_of_dof, p.vector("initial_guess"), faces
            s.ref = rr.refine(s.fc, s.flag)
            s.ref_u = rr.transfer(s.ref.forest, s.old_vertex, s.u_old, s.new_vertex, s.cons)
            steps.append(s)
        if cycle == last:
            break
        if family.endswith("-rnd"):
            x = rng.standard_normal(p.n_dofs())
        else:
            h = p.hierarchy()
            x = go.OracleMG(h, smoother=getattr(go, smoother)).solve(h.system_rhs, x0=p.vector("initial_guess"))["x"]
        p.finish_cycle_with(x)
        before = SimpleNamespace(name=f"{family}:{cycle}->{cycle + 1}", fc=fc, faces=faces, flag=p.refine_flags(), old_vertex=p.vertex_keys(),
                                 u_old=p.vector("solution"))
    p.close()
    return tuple(steps)


def step(name):
    family, rest = name.split(":")
    return _family(family)[int(rest.split("->")[0])]


# ------------------------------------------------------------------------------------------------ hand-built forests

def _hand(fc, where):
    """a step on a hand-built forest: random old values on its active vertices, the reference's new forest and numbering, and the
    constrained DoFs of tests/mesh_tables_reference.py (hanging and boundary vertices) zeroed"""
    flag = rr.flags_at(fc, where)
    ref = rr.refine(fc, flag)
    old_vertex, new_vertex = rr.active_vertices(fc), rr.active_vertices(ref.forest)
    u_old = np.random.default_rng(len(old_vertex)).standard_normal(len(old_vertex))
    cons = mtr.build(ref.forest).constraint_of_dof
    return SimpleNamespace(fc=fc, flag=flag, ref=ref, old_vertex=old_vertex, new_vertex=new_vertex, u_old=u_old, cons=cons,
                           ref_u=rr.transfer(ref.forest, old_vertex, u_old, new_vertex, cons))


def _inactive_only():
    fc = mtr.quadrant_2d()
    return _hand(fc, [(0, 0, 0, 0)])   # the refined cell: its flag does not count


HAND_BUILT = {
    "single-2d": lambda: _hand(rr.lattice(2, 1), [(0, 0, 0, 0)]),            # a new level appears
    "single-3d": lambda: _hand(rr.lattice(3, 1), [(0, 0, 0, 0)]),
    "lattice-2x2": lambda: _hand(rr.lattice(2, 2), [(0, 1, 0, 0)]),
    "staircase-2d": lambda: _hand(rr.staircase_2d(), [(2, 5, 5, 0)]),        # the closure adds flags on levels 1 and 0
    "edge-3d": lambda: _hand(mtr.edge_only_3d(), [(1, 1, 1, 1)]),            # a 3D closure: a level-1 flag forces level 0
    "inactive-only": _inactive_only,                                         # nothing is split
    "no-flags": lambda: _hand(rr.staircase_2d(), []),
    "zero-cells": lambda: _hand(mtr.empty(2), []),
}


@functools.lru_cache(maxsize=None)
def hand(name):
    return HAND_BUILT[name]()


def same_forest(got, ref, what=""):
    """arrays shaped like Context.get_refined_forest() against a forest namespace, cell for cell"""
    assert got.n_levels == ref.n_levels, (what, got.n_levels, ref.n_levels)
    assert np.array_equal(np.asarray(got.level_ptr), np.asarray(ref.level_ptr, dtype=np.int64)), (what, "level_ptr")
    assert np.array_equal(np.asarray(got.cell_coord).reshape(-1, 3), np.asarray(ref.cell_coord, dtype=np.int32).reshape(-1, 3)), (what, "cell_coord")
    assert np.array_equal(np.asarray(got.cell_first_child), np.asarray(ref.cell_first_child, dtype=np.int32)), (what, "cell_first_child")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
