"""The active-mesh system matrix restated from the exported assembly inputs (tests/system_matrix_reference.py) against the
host driver's assembly, bit for bit, on adaptively refined meshes with hanging-node and Dirichlet lines; and the argument
checks of the new entry points that need no device."""
import ctypes as C
import os

import numpy as np
import pytest

import system_matrix_reference as smr
from gpu_util import capi, pkg

# the golden atom files on a small box: 2 vacuum cells around the atoms, mesh size 0.25, exact boundary values
MESHES = [("atom_n1_8.data", 1.0, 4), ("atom_n3_216.data", 3.0, 3)]


def problem(golden_dir, name, right, cycles, **kw):
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=2, problem="GaussianCharges", dim=3, bc="Exact", cycles=cycles,
                             r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR", **kw))
    p.read_lammps(os.path.join(golden_dir, name))
    return p


def line_kinds(inp):
    """(edge lines, face lines, Dirichlet lines with nonzero inhomogeneity) of a set of assembly inputs"""
    n = np.diff(inp.line_ptr)
    first = inp.line_weight[np.minimum(inp.line_ptr[:-1], max(len(inp.line_weight) - 1, 0))] if len(inp.line_weight) else np.zeros(len(n))
    edge = int(np.sum((n > 0) & (first == 0.5)))
    face = int(np.sum((n > 0) & (first == 0.25)))
    dirichlet = int(np.sum((n == 0) & (inp.line_inhomogeneity != 0.0)))
    return edge, face, dirichlet


def oracle_solution(p):
    from oracle import gmg_oracle as go
    h = p.hierarchy()
    ref = go.OracleMG(h, smoother=go.SSOR).solve(h.system_rhs, x0=p.vector("initial_guess"))
    assert ref["status"] == go.OK
    return ref["x"]


@pytest.mark.parametrize("name,right,cycles", MESHES, ids=[m[0] for m in MESHES])
def test_reference_equals_host_assembly(golden_dir, name, right, cycles):
    p = problem(golden_dir, name, right, cycles)
    seen = np.zeros(3, dtype=np.int64)
    for cycle in range(cycles):
        p.run_cycle(cycle, on_device=False)
        inp = p.system_assembly_inputs()
        host = p.matrix("system")
        assert inp.n_dofs == host.n_rows == p.n_dofs() and inp.cell_dofs.shape[1] == 8
        ref = smr.assemble(inp)
        assert np.array_equal(ref.rowptr, host.rowptr), cycle
        assert np.array_equal(ref.col, host.col), cycle
        assert np.array_equal(ref.val.view(np.uint64), host.val.view(np.uint64)), cycle
        seen += line_kinds(inp)
        if cycle + 1 < cycles:
            p.finish_cycle_with(oracle_solution(p))
    # the comparison is about hanging nodes and Dirichlet lines: the meshes must have had them
    assert seen[0] > 0 and seen[1] > 0 and seen[2] > 0, seen
    p.close()


def test_array_and_loop_restatements_agree():
    inp = smr.quadrant_mesh_2d()
    assert np.sum(np.diff(inp.line_ptr) > 0) == 3 and inp.cell_dofs.shape == (12, 4)
    assert smr.same_bits(smr.assemble(inp), smr.assemble_loops(inp))


def test_key_defaults_to_host_assembly(golden_dir):
    """without the key nothing is left to the device; with it, a cycle that does not run on the device says so once and keeps
    the host path"""
    p = problem(golden_dir, "atom_n1_8.data", 1.0, 1)
    p.run_cycle(0, on_device=False)
    assert not p.system_matrix_on_device() and "System matrix on device" not in p.log()
    q = problem(golden_dir, "atom_n1_8.data", 1.0, 1, system_matrix_on_device=True)
    q.run_cycle(0, on_device=False)
    assert not q.system_matrix_on_device() and q.log().count("System matrix on device: not applicable") == 1
    assert smr.same_bits(p.matrix("system"), q.matrix("system"))
    p.close()
    q.close()


def test_null_context_is_refused():
    L = capi().load()
    assert L.gmg_assemble_system_matrix(None, C.c_int(3), C.c_int64(0), C.c_int64(0), None, None, None, None, C.c_int64(0), None, None, None, None) == capi().ERR_INVALID
    assert L.gmg_get_system_matrix(None, None, None, None, None, None) == capi().ERR_INVALID
    assert L.gmg_system_matrix_norms(None, None, None, None) == capi().ERR_INVALID


def test_python_side_validation():
    """the binding checks shapes before the library is called (a view of a null handle would otherwise be dereferenced)"""
    ctx = capi().Context.view(C.c_void_p())
    inp = smr.quadrant_mesh_2d()
    args = dict(dim=2, n_dofs=inp.n_dofs, cell_dofs=inp.cell_dofs, cell_level=inp.cell_level, K_of_level=inp.K_of_level,
                constraint_of_dof=inp.constraint_of_dof, line_ptr=inp.line_ptr, line_master=inp.line_master, line_weight=inp.line_weight)
    for bad in (dict(dim=4), dict(n_dofs=inp.n_dofs + 1), dict(cell_dofs=inp.cell_dofs[:, :3]), dict(K_of_level=inp.K_of_level[:15]),
                dict(line_master=inp.line_master[:-1]), dict(line_weight=inp.line_weight[:-2], line_master=inp.line_master[:-2])):
        with pytest.raises(ValueError):
            ctx.assemble_system_matrix(**dict(args, **bad))
