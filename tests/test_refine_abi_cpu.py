"""CPU-side checks of the boundary of "Refinement on device" (DESIGN.md section 21): the library exports the new entries, the
header defines them, the driver knows the key (default false) and its accessors work on the host path.  No GPU here."""
import os

import numpy as np

import refine_cases as rc
import refine_reference as rr
from gpu_util import capi, pkg
from test_system_matrix_cpu import problem as golden8_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gmg_refine_forest", "gmg_get_refined_forest", "gmg_transfer_solution", "gmg_build_face_table")


def test_library_exports_the_new_entries():
    pkg().build.build_device()
    lib = capi().load()
    header = open(os.path.join(ROOT, "include", "gmg_coulomb.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in capi().SYMBOLS and f"int {name}(gmg_context *ctx" in header, name
    for method in ("refine_forest", "get_refined_forest", "transfer_solution", "build_face_table"):
        assert callable(getattr(capi().Context, method))
    for cite in ("Forest::refine_flagged", "src/step-50.cc:1095-1100", "src/step-50.cc:1101-1121", "LaplaceProblem::face_table", "EQUAL plain stores"):
        assert cite in header, cite


def test_the_key_defaults_to_false_and_is_parsed():
    S = pkg().step50
    assert "set Refinement on device = true" in S.prm_text(refinement_on_device=True)
    p = golden8_problem(rc.mtc.GOLDEN, "atom_n1_8.data", 1.0, 2)
    p.run_cycle(0, on_device=False)
    p.finish_cycle_with(np.zeros(p.n_dofs()))
    p.run_cycle(1, on_device=False)
    assert not p.refined_on_device() and "Refinement on device" not in p.log()
    p.close()


def test_refine_with_flags_on_the_host_equals_the_reference():
    """Problem.refine_with_flags with marks of the test's own choosing, some on cells that are not active"""
    p = golden8_problem(rc.mtc.GOLDEN, "atom_n1_8.data", 1.0, 3)
    p.run_cycle(0, on_device=False)
    p.finish_cycle_with(np.sin(np.arange(p.n_dofs())))
    p.run_cycle(1, on_device=False)
    p.finish_cycle_with(np.sin(np.arange(p.n_dofs())))
    fc, old_vertex, u_old = p.forest_cells(), p.vertex_keys(), p.vector("solution")
    flag = np.zeros(len(fc.cell_first_child), dtype=np.uint8)
    flag[::5] = 1
    assert np.any(flag & (fc.cell_first_child >= 0)) and fc.n_levels == 2
    p.refine_with_flags(flag)
    ref = rr.refine(fc, flag)
    rc.same_forest(ref.forest, p.forest_cells())
    assert np.array_equal(np.asarray(ref.cell_parent, dtype=np.int32), p.forest_parents())
    assert np.array_equal(np.asarray(ref.closed_flag, dtype=np.uint8), p.closed_flags()) and ref.forest.n_levels == 3
    cons = p.system_assembly_inputs().constraint_of_dof
    assert np.array_equal(rc.bits(rr.transfer(ref.forest, old_vertex, u_old, p.vertex_keys(), cons)), rc.bits(p.vector("solution")))
    p.close()
