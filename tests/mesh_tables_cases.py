"""The meshes that tests/test_mesh_tables_cpu.py and tests/test_gpu_mesh_tables.py share: host runs of the driver, advanced
with the oracle's solutions, and per cycle the forest (Problem.forest_cells()), the host's arrays and the restatement of
tests/mesh_tables_reference.py -- computed once, left unchanged."""
import functools
import os
from types import SimpleNamespace

import numpy as np

import mesh_tables_reference as mtr
import mg_cases
from gpu_util import pkg
from test_coef_matrix_cpu import step16_problem
from test_system_matrix_cpu import problem as golden8_problem

GOLDEN = mg_cases.GOLDEN

#  name: (family, cycle).  A3 / B3: the adaptive hierarchies of tests/mg_cases.py; G8: the golden 8-atom file on the small box
#  of tests/test_system_matrix_cpu.py; S2 / S3: Step16 in 2D (3 global refinements) and 3D (2 global refinements), Kelly
#  marking; CW: G8 with "Level 0 numbering = cell-wise"
CASES = {"A3": ("A3", 3), "B3": ("B3", 3), "G8-c0": ("G8", 0), "G8-c1": ("G8", 1), "G8-c2": ("G8", 2), "S2-c1": ("S2", 1), "S2-c2": ("S2", 2),
         "S3-c1": ("S3", 1), "CW-c1": ("CW", 1)}


def _open(family):
    """(problem, smoother, origin, h0): lower-left corner and root cell size as make_initial_grid derives them"""
    S = pkg().step50
    if family in mg_cases.ADAPTIVE:
        vac, mesh, bc, last = mg_cases.ADAPTIVE[family][:4]
        p = S.Problem(S.prm_text(left=0, right=1, mesh_size=mesh, vacuum=vac, problem="GaussianCharges", dim=3, bc=bc, cycles=last + 1, r_c=0.5,
                                 cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR"))
        p.read_lammps(os.path.join(GOLDEN, "atom_n1_2.data"))
        return p, "SSOR", _lattice_geometry(0.0, 1.0, mesh, vac)
    if family in ("G8", "CW"):
        kw = dict(level0_numbering="cell-wise") if family == "CW" else {}
        return golden8_problem(GOLDEN, "atom_n1_8.data", 1.0, 3, **kw), "SSOR", _lattice_geometry(0.0, 1.0, 0.25, 2)
    return step16_problem(2 if family == "S2" else 3, 3 if family == "S2" else 2, 3), "JACOBI", (0.0, 1.0)


def _lattice_geometry(left, right, mesh, vac):
    a = 2 * mesh
    reps = int(2 * ((right - left) / a + 2 * vac))
    lo, hi = left - vac * a, right + vac * a
    return lo, (hi - lo) / reps


@functools.lru_cache(maxsize=None)
def _cycles(family):
    from oracle import gmg_oracle as go

    last = max(c for f, c in CASES.values() if f == family)
    p, smoother, (origin, h0) = _open(family)
    out = []
    for cycle in range(last + 1):
        p.run_cycle(cycle, on_device=False)
        fc = p.forest_cells()
        snap = SimpleNamespace(fc=fc, sys=p.system_assembly_inputs(), levels=[p.level_assembly_inputs(l) for l in range(p.n_levels())],
                               xyz=p.dof_coordinates(), origin=origin, h0=h0, ref=mtr.build(fc))
        out.append(snap)
        if cycle < last:
            h = p.hierarchy()
            p.finish_cycle_with(go.OracleMG(h, smoother=getattr(go, smoother)).solve(h.system_rhs, x0=p.vector("initial_guess"))["x"])
    p.close()
    return tuple(out)


def case(name):
    family, cycle = CASES[name]
    return _cycles(family)[cycle]


HAND_BUILT = {"single-2d": lambda: mtr.single_cell(2), "single-3d": lambda: mtr.single_cell(3), "single-3d-cellwise": lambda: mtr.single_cell(3, False),
              "empty-2d": lambda: mtr.empty(2), "empty-3d": lambda: mtr.empty(3), "quadrant-2d": mtr.quadrant_2d,
              "quadrant-2d-cellwise": lambda: mtr.quadrant_2d(False), "edge-only-3d": mtr.edge_only_3d}


def same_tables(got, ref, what=""):
    """the arrays of Context.get_mesh_tables / get_mesh_level_tables (or anything shaped like them) against build()'s lists"""
    for k in ("n_cells", "n_dofs", "n_hanging", "n_lines"):
        assert getattr(got, k) == getattr(ref, k), (what, k, getattr(got, k), getattr(ref, k))
    nv = len(ref.cell_dofs[0]) if ref.n_cells else 1
    assert np.array_equal(np.asarray(got.cell_dofs).reshape(-1, nv), np.asarray(ref.cell_dofs, dtype=np.int32).reshape(-1, nv)), (what, "cell_dofs")
    for k, dt in (("cell_level", np.uint8), ("vertex_of_dof", np.uint64), ("constraint_of_dof", np.int32), ("line_ptr", np.int64), ("line_master", np.int32),
                  ("line_dof", np.int32)):
        assert np.array_equal(np.asarray(getattr(got, k)), np.asarray(getattr(ref, k), dtype=dt)), (what, k)
    assert np.array_equal(np.asarray(got.line_weight).view(np.uint64), np.asarray(ref.line_weight, dtype=np.float64).view(np.uint64)), (what, "line_weight")


def same_level(got, ref, what=""):
    assert got.n_cells == ref.n_cells and got.n_dofs == ref.n_dofs, (what, got.n_cells, got.n_dofs, ref.n_cells, ref.n_dofs)
    nv = len(ref.cell_dofs[0]) if ref.n_cells else 1
    assert np.array_equal(np.asarray(got.cell_dofs).reshape(-1, nv), np.asarray(ref.cell_dofs, dtype=np.int32).reshape(-1, nv)), (what, "cell_dofs")
    assert np.array_equal(np.asarray(got.vertex_of_dof), np.asarray(ref.vertex_of_dof, dtype=np.uint64)), (what, "vertex_of_dof")
    assert np.array_equal(np.asarray(got.dof_flags), np.asarray(ref.dof_flags, dtype=np.uint8)), (what, "dof_flags")
