"""The eight entries of "Operators from resident tables"  in the header and the library, the prm key's
default, and a host cycle with the key set.  Needs no GPU."""
import ctypes as C
import os
import re

import numpy as np

from gpu_util import capi, pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gmg_close_constraints", "gmg_get_closed_constraints", "gmg_assemble_system_matrix_resident", "gmg_assemble_system_matrix_coef_resident",
       "gmg_assemble_level_matrix_resident", "gmg_assemble_level_matrix_coef_resident", "gmg_assemble_rhs_resident",
       "gmg_distribute_constraints_resident")


def test_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "gmg_coulomb.h")).read()
    declared = set(re.findall(r"\b(gmg_[a-z0-9_]+)\s*\(", text))
    L = capi().load()
    for s in NEW:
        assert s in declared, s
        assert s in capi().SYMBOLS, s
        assert hasattr(L, s), s


def test_null_context_is_refused():
    A = capi()
    L = A.load()
    assert L.gmg_close_constraints(None, C.c_int64(0), None, None) == A.ERR_INVALID
    assert L.gmg_get_closed_constraints(None, None, None, None, None, None, None) == A.ERR_INVALID
    assert L.gmg_assemble_system_matrix_resident(None, None, None) == A.ERR_INVALID
    assert L.gmg_assemble_system_matrix_coef_resident(None, C.c_int(1), None, None, None, None, None) == A.ERR_INVALID
    assert L.gmg_assemble_level_matrix_resident(None, C.c_int(0), None, None) == A.ERR_INVALID
    assert L.gmg_assemble_level_matrix_coef_resident(None, C.c_int(0), C.c_int(1), None, None, None, C.c_double(1.0), None) == A.ERR_INVALID
    assert L.gmg_assemble_rhs_resident(None, None, C.c_int(1), None, None, None, None, None, None) == A.ERR_INVALID
    assert L.gmg_distribute_constraints_resident(None, C.c_int64(0), None) == A.ERR_INVALID


def test_key_defaults_to_false_and_leaves_a_host_cycle_alone():
    S = pkg().step50
    args = dict(left=-1, right=1, mesh_size=0.25, vacuum=1, problem="GaussianCharges", dim=2, bc="Homogeneous", cycles=1, r_c=0.5, global_refinement=0)
    assert "resident" not in S.prm_text(**args)
    assert "set Operators from resident tables = true" in S.prm_text(operators_from_resident_tables=True, **args)
    p = S.Problem(S.prm_text(**args))
    p.run_cycle(0, on_device=False)
    assert not p.operators_resident() and "Operators from resident tables" not in p.log()
    # the key alone, and with every prerequisite key, on a cycle without a device: the host path, and one line that says why
    for more in ({}, dict(mesh_tables_on_device=True, system_matrix_on_device=True, level_matrices_on_device=True, rhs_from_cell_tables=True)):
        q = S.Problem(S.prm_text(operators_from_resident_tables=True, **more, **args))
        q.run_cycle(0, on_device=False)
        assert not q.operators_resident()
        assert q.log().count("Operators from resident tables: not applicable (the mesh tables were not formed on the device), host arrays") == 1
        a, b = p.system_assembly_inputs(), q.system_assembly_inputs()
        for k in ("cell_dofs", "cell_level", "constraint_of_dof", "line_ptr", "line_master"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert np.array_equal(a.line_weight.view(np.uint64), b.line_weight.view(np.uint64))
        assert np.array_equal(a.line_inhomogeneity.view(np.uint64), b.line_inhomogeneity.view(np.uint64))
        assert np.array_equal(p.vector("rhs").view(np.uint64), q.vector("rhs").view(np.uint64))
        hp, hq = p.hierarchy(), q.hierarchy()
        assert np.array_equal(hp.system_matrix.val.view(np.uint64), hq.system_matrix.val.view(np.uint64))
        q.close()
    p.close()
