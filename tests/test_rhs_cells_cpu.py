"""The right-hand side restated from the exported cell tables (tests/rhs_cells_reference.py: the definition of gmg_assemble_rhs
in plain loops) against the host driver's system_rhs, bit for bit, on adaptively refined meshes with hanging-node lines and
nonzero Dirichlet values; constraints.distribute restated likewise against the host's distributed solution; the precondition
of gmg_distribute_constraints on every mesh; and the argument checks that need no device.  Needs no GPU."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import mg_cases
import rhs_cells_reference as rcr
from gpu_util import capi, pkg
from test_coef_matrix_cpu import step16_problem
from test_system_matrix_cpu import problem as golden8_problem

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

#  name: (family, cycle).  A3 / B3: the adaptive hierarchies of tests/mg_cases.py (2 atoms; Exact / Inhomogeneous boundary values);
#  G8: the golden 8-atom file on the small box of tests/test_system_matrix_cpu.py; S2 / S3: Step16 in 2D (3 global refinements)
#  and 3D (2 global refinements), Kelly marking
CASES = {"A3": ("A3", 3), "B3": ("B3", 3), "G8-c0": ("G8", 0), "G8-c1": ("G8", 1), "G8-c2": ("G8", 2), "S2-c1": ("S2", 1), "S3-c1": ("S3", 1)}
#  what the cases held when they were chosen: (DoFs, cells, hanging-node lines, cells with a nonzero Dirichlet term, cells with both
#  a hanging node and such a term, DoFs that are master of more than one line).  Only A3 refines up to the boundary: it is the case
#  with cells that have both.
EXPECTED = {"A3": (2008, 1436, 428, 538, 110, 137), "B3": (2794, 2064, 744, 488, 0, 252), "G8-c0": (2197, 1728, 0, 728, 0, 0),
            "G8-c1": (2685, 1952, 432, 728, 0, 160), "G8-c2": (3641, 2680, 936, 728, 0, 304), "S2-c1": (238, 205, 16, 0, 0, 12),
            "S3-c1": (388, 225, 117, 0, 0, 23)}


def _open(family):
    S = pkg().step50
    if family in mg_cases.ADAPTIVE:
        vac, mesh, bc, last = mg_cases.ADAPTIVE[family][:4]
        p = S.Problem(S.prm_text(left=0, right=1, mesh_size=mesh, vacuum=vac, problem="GaussianCharges", dim=3, bc=bc, cycles=last + 1, r_c=0.5,
                                 cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR"))
        p.read_lammps(os.path.join(GOLDEN, "atom_n1_2.data"))
        return p, "SSOR"
    if family == "G8":
        return golden8_problem(GOLDEN, "atom_n1_8.data", 1.0, 3), "SSOR"
    return step16_problem(2 if family == "S2" else 3, 3 if family == "S2" else 2, 2), "JACOBI"


@functools.lru_cache(maxsize=None)
def _cycles(family):
    """per cycle of a host run: namespace(inp, rhs, x, sol) -- the exported inputs, the host's system_rhs, the oracle's solution
    as the solver left it and the host's solution after constraints.distribute"""
    from oracle import gmg_oracle as go

    last = max(c for f, c in CASES.values() if f == family)
    p, smoother = _open(family)
    out = []
    for cycle in range(last + 1):
        p.run_cycle(cycle, on_device=False)
        inp, rhs, h = p.rhs_assembly_inputs(), p.vector("rhs"), p.hierarchy()
        x = go.OracleMG(h, smoother=getattr(go, smoother)).solve(h.system_rhs, x0=p.vector("initial_guess"))["x"]
        p.finish_cycle_with(x)
        snap = SimpleNamespace(inp=inp, rhs=rhs, x=np.array(x), sol=p.vector("solution"))
        for v in (snap.rhs, snap.x, snap.sol, inp.source):
            v.setflags(write=False)
        out.append(snap)
    p.close()
    return tuple(out)


def case(name):
    family, cycle = CASES[name]
    return _cycles(family)[cycle]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restated right-hand side of a case: computed once, shared with the GPU tests"""
    ref = rcr.assemble(case(name).inp)
    ref.setflags(write=False)
    return ref


def coverage(name):
    inp = case(name).inp
    return (inp.n_dofs, len(inp.cell_level)) + rcr.features(inp)


@pytest.mark.parametrize("name", CASES)
def test_cases_hold_what_the_comparison_is_about(name):
    """hanging-node lines, cells with a nonzero Dirichlet term, cells with both, and DoFs that are master of several lines --
    where the case has them; a drifting mesh must not silently empty the tests"""
    got = coverage(name)
    print(name, got)
    n_dofs, cells, hanging, dirichlet, both, multi = got
    family = CASES[name][0]
    if name in ("A3", "B3", "G8-c1", "G8-c2"):
        assert hanging > 0 and dirichlet > 0 and multi > 0, got
    if name == "A3":
        assert both > 0, got
    if family in ("S2", "S3"):
        assert hanging > 0 and dirichlet == 0 and multi > 0, got    # Step16: homogeneous boundary values
    if name == "G8-c0":
        assert hanging == 0 and dirichlet > 0, got    # the unrefined lattice
    assert got == EXPECTED[name]


@pytest.mark.parametrize("name", CASES)
def test_reference_equals_host_rhs(name):
    x = case(name)
    inp = x.inp
    assert inp.n_dofs == len(x.rhs) and inp.source.shape == (len(inp.cell_level), inp.nq) and inp.shape.shape == (inp.nq, 1 << inp.dim)
    assert np.any(x.rhs != 0.0)
    assert rcr.same_bits(reference(name), x.rhs), name


@pytest.mark.parametrize("name", CASES)
def test_no_master_is_constrained(name):
    """the precondition under which one thread per constrained DoF agrees with the host's ascending in-place loop"""
    assert rcr.masters_unconstrained(case(name).inp)


@pytest.mark.parametrize("name", CASES)
def test_reference_distribution_equals_the_host(name):
    x = case(name)
    ref = rcr.distribute(x.inp, x.x)
    assert rcr.same_bits(ref, x.sol), name
    if CASES[name][0] != "S2" and CASES[name][0] != "S3":
        assert np.any(ref != x.x)  # constrained entries received values


def test_step16_source_is_exported_once_per_point():
    """the source of a Step16 mesh: one finite value per quadrature point, the same bits in a second export (one cell per
    iteration: no dependence on the threads), and the host's right-hand side from them"""
    p = step16_problem(2, 3, 1)
    p.run_cycle(0, on_device=False)
    a, b = p.rhs_assembly_inputs(), p.rhs_assembly_inputs()
    assert a.source.shape == (64, a.nq) and np.all(np.isfinite(a.source)) and np.any(a.source != 0.0) and rcr.same_bits(a.source, b.source)
    assert rcr.same_bits(rcr.assemble(a), p.vector("rhs"))
    p.close()


def test_key_defaults_to_the_host_pass():
    """without the key nothing changes; with it, a cycle that does not run on the device says so once and keeps the host pass"""
    p = golden8_problem(GOLDEN, "atom_n1_8.data", 1.0, 1)
    p.run_cycle(0, on_device=False)
    assert not p.rhs_from_cell_tables() and "RHS from cell tables" not in p.log()
    q = golden8_problem(GOLDEN, "atom_n1_8.data", 1.0, 1, rhs_from_cell_tables=True)
    q.run_cycle(0, on_device=False)
    assert not q.rhs_from_cell_tables() and q.log().count("RHS from cell tables: not applicable") == 1
    assert rcr.same_bits(p.vector("rhs"), q.vector("rhs"))
    p.close()
    q.close()


def test_null_context_is_refused():
    L = capi().load()
    assert L.gmg_assemble_rhs(None, C.c_int(3), C.c_int64(0), C.c_int64(0), None, None, None, C.c_int64(0), None, None, None, None, None, C.c_int(1),
                              None, None, None, None, None, None) == capi().ERR_INVALID
    assert L.gmg_distribute_constraints(None, C.c_int64(0), None, None, C.c_int64(0), None, None, None, None) == capi().ERR_INVALID
