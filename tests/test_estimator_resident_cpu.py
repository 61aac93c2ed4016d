"""The CPU side of "Estimator from resident tables" (DESIGN.md section 24): the new symbols, the prm key and its fallback on a
host cycle, the plain-numpy restatement of "flags from marks" against the host's refine_flags on every step of
tests/refine_cases.py, and the properties of those steps that let the GPU tests catch a wrong kernel."""
import ctypes as C
import os
import re

import numpy as np

import estimator_resident_cases as erc
import mesh_tables_cases as mtc
import mesh_tables_reference as mtr
import refine_cases as rc
import refine_reference as rr
from gpu_util import capi, pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gmg_build_face_table_resident", "gmg_get_face_table", "gmg_estimate_error_resident", "gmg_get_marks", "gmg_refine_forest_marked",
       "gmg_energy_norm_error_resident"]
LINE = "   Estimator from resident tables: not applicable ({}), host arrays"


def test_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "gmg_coulomb.h")).read()
    declared = set(re.findall(r"\b(gmg_[a-z0-9_]+)\s*\(", text))
    A = capi()
    L = A.load()
    for s in NEW:
        assert s in declared and s in A.SYMBOLS and hasattr(L, s), s
    for m in ("build_face_table_resident", "get_face_table", "estimate_error_resident", "get_marks", "refine_forest_marked", "energy_norm_error_resident"):
        assert callable(getattr(A.Context, m)), m
    assert hasattr(pkg().step50.load(), "step50_estimator_resident")
    # a NULL context is refused before anything else is read
    assert L.gmg_get_face_table(None, None, None, None) == A.ERR_INVALID
    assert L.gmg_get_marks(None, None, None, None) == A.ERR_INVALID
    assert L.gmg_build_face_table_resident(None, C.c_int(2), None, C.c_int(0), None, None, None, None, None) == A.ERR_INVALID
    assert L.gmg_refine_forest_marked(None, C.c_int(2), None, C.c_int(0), None, None, None, None, None, None, None) == A.ERR_INVALID


def test_key_defaults_to_false_and_a_host_cycle_says_why():
    S = pkg().step50
    args = dict(left=0, right=1, mesh_size=0.25, vacuum=1, problem="GaussianCharges", dim=3, bc="Homogeneous", cycles=2, r_c=0.5, global_refinement=0)
    assert "Estimator from resident tables" not in S.prm_text(**args)
    assert "set Estimator from resident tables = true" in S.prm_text(estimator_from_resident_tables=True, **args)
    golden = os.path.join(mtc.GOLDEN, "atom_n1_8.data")
    runs = []
    for more in ({}, dict(estimator_from_resident_tables=True),
                 dict(estimator_from_resident_tables=True, estimator_on_device=True, refinement_on_device=True, operators_from_resident_tables=True)):
        p = S.Problem(S.prm_text(**more, **args))
        p.read_lammps(golden)
        p.run_cycle(0, on_device=False)
        p.finish_cycle_with(np.cos(np.arange(p.n_dofs())))
        p.run_cycle(1, on_device=False)
        assert not p.estimator_resident()
        runs.append((p.log(), p.refine_flags(), p.error_per_cell(), p.vector("initial_guess"), p.forest_cells()))
        p.close()
    assert "Estimator from resident tables" not in runs[0][0]   # the default is false: nothing is said
    for log, flags, eta, guess, fc in runs[1:]:
        assert log.count(LINE.format("Operators from resident tables did not take effect")) == 1, log   # once over two cycles
        assert np.array_equal(flags, runs[0][1]) and np.array_equal(eta.view(np.uint32), runs[0][2].view(np.uint32))
        assert np.array_equal(guess.view(np.uint64), runs[0][3].view(np.uint64))
        rc.same_forest(fc, runs[0][4])


def between_marked(fc, flag):
    """is there an inactive cell whose position in the flag array lies between two marked active cells?"""
    flag = np.asarray(flag).reshape(-1) != 0
    active = np.asarray(fc.cell_first_child).reshape(-1) < 0
    hit = np.flatnonzero(flag & active)
    return len(hit) >= 2 and bool((~active[hit[0]:hit[-1]]).any())


def sandwich_2d():
    """2 x 2 roots, root (0, 0) refined, its child (1, 0) refined again: level 1 starts [active, INACTIVE, active, active]"""
    fc = rr.refined(rr.lattice(2, 2), [(0, 0, 0, 0)], [(1, 1, 0, 0)])
    return fc, rr.flags_at(fc, [(1, 0, 0, 0), (1, 0, 1, 0), (2, 2, 0, 0)])


def test_flags_from_marks_on_every_step():
    """the restatement of gmg_refine_forest_marked's flags reproduces the host's refine_flags from its marks"""
    n = 0
    for name in rc.STEPS:
        s = rc.step(name)
        marks = erc.marks_of_flags(s.fc, s.flag)
        assert np.array_equal(erc.flags_from_marks(s.fc, marks), np.asarray(s.flag, dtype=np.uint8)), name   # (no flag sits on an inactive cell)
        # the active number is the row of the host's face table: a kind-1 neighbour's neighbour across the same face is the cell
        kind, cell = np.asarray(s.faces[0]), np.asarray(s.faces[1])
        assert kind.shape[0] == len(marks), name
        a, f = np.nonzero(kind == 1)
        back = cell.reshape(kind.shape[0], kind.shape[1], -1)[cell.reshape(kind.shape[0], kind.shape[1], -1)[a, f, 0], f ^ 1, 0]
        assert np.array_equal(back, a), name
        n += 1
    assert n == len(rc.STEPS) >= 10
    for name in sorted(rc.HAND_BUILT):
        s = rc.hand(name)
        marks = erc.marks_of_flags(s.fc, s.flag)
        want = np.asarray(s.flag, dtype=np.uint8).reshape(-1) * (np.asarray(s.fc.cell_first_child, dtype=np.int64).reshape(-1) < 0)
        assert np.array_equal(erc.flags_from_marks(s.fc, marks), want), name


def test_the_driver_s_marks_give_its_flags():
    """a host cycle of the driver: Problem.marks() (per active cell) through the restatement is Problem.refine_flags()"""
    p, _, _ = mtc._open("G8")
    p.run_cycle(0, on_device=False)
    p.finish_cycle_with(np.cos(np.arange(p.n_dofs())))   # (the estimator runs on this vector)
    marks, flags, fc = p.marks(), p.refine_flags(), p.forest_cells()
    p.close()
    assert 0 < marks.sum() < len(marks)
    assert np.array_equal(erc.flags_from_marks(fc, marks), np.asarray(flags, dtype=np.uint8))


def test_the_cases_can_catch_a_wrong_kernel():
    kinds = {2: np.zeros(4, dtype=np.int64), 3: np.zeros(4, dtype=np.int64)}
    partial = grows = between = False
    for name in rc.STEPS:
        s = rc.step(name)
        kinds[s.fc.dim] += np.bincount(np.asarray(s.faces[0]).ravel(), minlength=4)[:4]
        marks = erc.marks_of_flags(s.fc, s.flag)
        partial |= 0 < marks.sum() < len(marks)
        grows |= bool((np.asarray(s.closed) > np.asarray(s.flag)).any())
        between |= between_marked(s.fc, s.flag)
    assert np.all(kinds[2] > 0) and np.all(kinds[3] > 0), kinds   # face kinds 0, 1, 2 and 3, in 2D and in 3D
    assert partial and grows
    fc, flag = sandwich_2d()   # (held whether or not a driven step has one: the GPU tests run this forest too)
    assert between_marked(fc, flag) and mtr.build(fc).n_cells == int((np.asarray(fc.cell_first_child) < 0).sum())
    assert between or between_marked(fc, flag)
