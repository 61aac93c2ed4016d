"""The meshes tests/test_gpu_resident.py takes: host runs of the driver, advanced with the oracle's solutions, and of the chosen
cycle everything the device entries consume -- the forest, the host's cell tables and closed lines, the level inputs, the
right-hand side's inputs, the hierarchy (copy lists, transfers) and, for Step16, the coefficient inputs.  Computed once."""
import functools
import os
from types import SimpleNamespace

import mg_cases
from gpu_util import pkg
from test_coef_matrix_cpu import step16_problem

GOLDEN = mg_cases.GOLDEN

#  A3 / B3: the adaptive hierarchies of tests/mg_cases.py (level rows 729 / 1303 / 250 and 1331 / 827 / 941; Exact / Inhomogeneous
#  boundary values); S2-c2: Step16 in 2D refined twice; S3-c1: Step16 in 3D, cycle 1
CASES = {"A3": ("A3", 3), "B3": ("B3", 3), "S2-c2": ("S2", 2), "S3-c1": ("S3", 1)}
STEP16 = ("S2-c2", "S3-c1")


def _open(family):
    S = pkg().step50
    if family in mg_cases.ADAPTIVE:
        vac, mesh, bc, last = mg_cases.ADAPTIVE[family][:4]
        p = S.Problem(S.prm_text(left=0, right=1, mesh_size=mesh, vacuum=vac, problem="GaussianCharges", dim=3, bc=bc, cycles=last + 1, r_c=0.5,
                                 cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR"))
        p.read_lammps(os.path.join(GOLDEN, "atom_n1_2.data"))
        return p, "SSOR"
    return step16_problem(2 if family == "S2" else 3, 3 if family == "S2" else 2, 3), "JACOBI"


@functools.lru_cache(maxsize=None)
def case(name):
    from oracle import gmg_oracle as go

    family, last = CASES[name]
    p, smoother = _open(family)
    for cycle in range(last + 1):
        p.run_cycle(cycle, on_device=False)
        if cycle < last:
            h = p.hierarchy()
            p.finish_cycle_with(go.OracleMG(h, smoother=getattr(go, smoother)).solve(h.system_rhs, x0=p.vector("initial_guess"))["x"])
    L = p.n_levels()
    x = SimpleNamespace(fc=p.forest_cells(), sys=p.system_assembly_inputs(), rhs=p.rhs_assembly_inputs(),
                        levels=[p.level_assembly_inputs(l) for l in range(L)], h=p.hierarchy(), host_rhs=p.vector("rhs"))
    if name in STEP16:
        x.sysc, x.levc = p.system_coefficient_inputs(), [p.level_coefficient_inputs(l) for l in range(L)]
    p.close()
    if family in mg_cases.ADAPTIVE:   # a drifting mesh must not silently empty the tests
        assert [lv.n_dofs for lv in x.levels] == mg_cases.ADAPTIVE[family][4]
    return x
