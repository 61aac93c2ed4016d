"""The graphical output of a cycle (csrc/host/output.inc; the reference's output_results,
src/step-50.cc:1149-1308) on host-only cycles: the three files parse, the patch arrays equal the restatement of
tests/output_reference.py bit for bit, the cell vectors are the estimator's, the optional arrays follow the reference's three
output keys, and nothing is written -- and no log line added -- while "Output results" is off."""
import functools
import math
import os

import numpy as np
import pytest

import mesh_tables_cases as mtc
import output_reference as ore
from gpu_util import pkg
from test_coef_matrix_cpu import step16_problem
from test_system_matrix_cpu import problem as golden8_problem

GOLDEN = mtc.GOLDEN

#  family: (dim, cycles, smoother of the oracle's solve, (origin, h0) as make_initial_grid derives them)
FAMILIES = {"G8": (3, 3, "SSOR", mtc._lattice_geometry(0.0, 1.0, 0.25, 2)), "S2": (2, 3, "JACOBI", (0.0, 1.0))}


def open_family(family, **kw):
    if family == "G8":
        return golden8_problem(GOLDEN, "atom_n1_8.data", 1.0, 3, **kw)
    return step16_problem(2, 3, 3, **kw)


@functools.lru_cache(maxsize=None)
def oracle_solutions(family):
    """the oracle's solution of every cycle of a family (a run with the key off), and that run's log"""
    from oracle import gmg_oracle as go

    _, cycles, smoother, _ = FAMILIES[family]
    p = open_family(family)
    out = []
    for cycle in range(cycles):
        p.run_cycle(cycle, on_device=False)
        h = p.hierarchy()
        out.append(go.OracleMG(h, smoother=getattr(go, smoother)).solve(h.system_rhs, x0=p.vector("initial_guess"))["x"])
        p.finish_cycle_with(out[-1])
    log = p.log()
    p.close()
    return tuple(out), log


def run_family(family, directory, each_cycle=None, **kw):
    """the same cycles with "Output results" set, writing into directory; each_cycle(p, cycle) after every finish_cycle"""
    xs, _ = oracle_solutions(family)
    p = open_family(family, output_results=True, output_directory=str(directory), **kw)
    for cycle, x in enumerate(xs):
        p.run_cycle(cycle, on_device=False)
        p.finish_cycle_with(x)
        if each_cycle:
            each_cycle(p, cycle)
    log = p.log()
    p.close()
    return log


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_files_hold_the_restated_patches(family, tmp_path):
    dim, cycles, _, (origin, h0) = FAMILIES[family]
    nv = 1 << dim
    hanging = []

    def check(p, cycle):
        inp = p.system_assembly_inputs()
        n_cells = len(inp.cell_level)
        hanging.append(len(np.unique(inp.cell_level)) > 1)
        piece, pvtu, visit = ore.names(cycle)
        f = ore.read_vtu(os.path.join(tmp_path, piece))
        assert f.n_cells == n_cells and f.n_points == nv * n_cells and f.cell_data == []
        conn, offsets, types = ore.connectivity(dim, n_cells)
        assert f.connectivity.dtype.kind == "i" and np.array_equal(f.connectivity, conn) and np.array_equal(f.offsets, offsets) and np.array_equal(f.types, types)
        ref = ore.patches(dim, inp.cell_dofs, inp.cell_level, p.vertex_keys(), origin, h0, p.vector("solution"))
        assert ore.same_bits(f.points, ref.point)
        assert ore.same_bits(f.point_data["solution"], ref.solution)
        assert ore.same_bits(f.point_data["grad_phi"], ref.grad_phi)
        # the points are the driver's vertex coordinates, so the copies of a vertex in neighbouring cells coincide exactly
        assert ore.same_bits(f.points, p.dof_coordinates()[np.asarray(inp.cell_dofs).reshape(-1)])
        assert list(f.point_data) == ["solution", "grad_phi", "subdomain", "error_indicator"]
        assert f.point_types == {"solution": ("Float64", 1), "grad_phi": ("Float64", 3), "subdomain": ("Float32", 1), "error_indicator": ("Float32", 1)}
        assert f.point_data["error_indicator"].tobytes() == np.repeat(p.error_per_cell(), nv).tobytes()
        assert f.point_data["subdomain"].tobytes() == np.zeros(nv * n_cells, dtype=np.float32).tobytes()
        # Problem.output_patches: the host mirror itself
        pt, sol, g = p.output_patches(on_device=False)
        assert ore.same_bits(pt, ref.point) and ore.same_bits(sol, ref.solution) and ore.same_bits(g, ref.grad_phi)
        pv = ore.read_pvtu(os.path.join(tmp_path, pvtu))
        assert pv.pieces == [piece] and pv.points == ("Float64", 3) and pv.point_types == f.point_types and list(pv.point_types) == list(f.point_data)
        with open(os.path.join(tmp_path, visit)) as fh:
            assert fh.read() == "!NBLOCKS 1\n" + piece + "\n"

    log = run_family(family, tmp_path, check)
    assert hanging[0] is False and hanging[-1] is True   # uniform first, hanging nodes later
    assert sorted(os.listdir(tmp_path)) == sorted(n for c in range(cycles) for n in ore.names(c))
    # the one line the key adds to the log says where the patches were formed
    extra = [l for l in log.splitlines() if "Output results" in l]
    assert extra == ["   Output results: patches formed on the host (the cycle does not run on the device)"]


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_key_off_writes_nothing_and_changes_no_log(family, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)   # (the default directory is the working directory)
    xs, log_off = oracle_solutions(family)
    p = open_family(family, output_directory=str(tmp_path))
    for cycle, x in enumerate(xs):
        p.run_cycle(cycle, on_device=False)
        p.finish_cycle_with(x)
    assert os.listdir(tmp_path) == []
    assert p.log() == log_off and "Output results" not in log_off
    # an explicit call works without the key
    assert p.output_results(7, str(tmp_path / "explicit")) == 0
    assert sorted(os.listdir(tmp_path / "explicit")) == sorted(ore.names(7))
    p.close()
    log_on = run_family(family, tmp_path / "on")
    assert [l for l in log_on.splitlines() if "Output results" not in l] == log_off.splitlines()


def test_a_second_run_writes_identical_bytes(tmp_path):
    run_family("G8", tmp_path / "a")
    run_family("G8", tmp_path / "b")
    for cycle in range(FAMILIES["G8"][1]):
        assert ore.read_bytes(tmp_path / "a", cycle) == ore.read_bytes(tmp_path / "b", cycle)


# ------------------------------------------------------------------------------------------------ the optional arrays

def two_atom_problem(tmp_path, **kw):
    S = pkg().step50
    args = dict(left=0, right=1, mesh_size=0.25, vacuum=2, problem="GaussianCharges", dim=3, bc="Exact", cycles=2, r_c=0.5, cutoff=3.5, rhs_optimization=True,
                quad_rhs=1, global_refinement=0, smoother="SSOR", output_results=True, output_directory=str(tmp_path), output_analytical=True,
                output_rhs_field=True, output_atom_support=True)
    args.update(kw)
    p = S.Problem(S.prm_text(**args))
    p.read_lammps(os.path.join(GOLDEN, "atom_n1_2.data"))
    return p


def support_reference(p, inp, origin, h0, cut):
    """per atom, 1 where the atom passes the list predicate of the charge densities for the cell: its distance to the nearest
    vertex of the cell's ROOT cell, direction by direction, is below the cutoff (children inherit the root's list)"""
    q, x = p.atoms()
    fc = p.forest_cells()
    level_of = np.repeat(np.arange(fc.n_levels), np.diff(fc.level_ptr))
    active = np.flatnonzero(np.asarray(fc.cell_first_child) < 0)
    assert np.array_equal(level_of[active], inp.cell_level)
    root = np.asarray(fc.cell_coord)[active] >> level_of[active][:, None]
    lo = origin + h0 * root.astype(np.float64)
    hi = origin + h0 * (root + 1).astype(np.float64)
    out = []
    for xi in x:
        dl, dh = xi[None, :] - lo, xi[None, :] - hi
        m = np.where(np.abs(dl) <= np.abs(dh), dl, dh)
        d2 = np.zeros(len(lo))
        for d in range(3):
            d2 = d2 + m[:, d] * m[:, d]
        out.append((np.sqrt(d2) < cut).astype(np.float32))
    return out


def test_optional_arrays_on_the_two_atom_input(tmp_path):
    from oracle import gmg_oracle as go

    origin, h0 = mtc._lattice_geometry(0.0, 1.0, 0.25, 2)
    r_c = 0.5
    p = two_atom_problem(tmp_path)
    for cycle in range(2):
        p.run_cycle(cycle, on_device=False)
        h = p.hierarchy()
        p.finish_cycle_with(go.OracleMG(h, smoother=go.SSOR).solve(h.system_rhs, x0=p.vector("initial_guess"))["x"])
        inp = p.system_assembly_inputs()
        cd = np.asarray(inp.cell_dofs).reshape(-1)
        f = ore.read_vtu(os.path.join(tmp_path, ore.names(cycle)[0]))
        assert list(f.point_data) == ["solution", "grad_phi", "Analytical_Solution_atoms", "interpolated_rhs", "support_0", "support_1", "subdomain",
                                      "error_indicator"]
        X = p.dof_coordinates()
        q, x = p.atoms()
        # Analytical_Solution::value (include/step_50.h:338-353) at the DoFs; the tolerance of tests/test_exact_solution_cpu.py
        ref = np.zeros(len(X))
        for qi, xi in zip(q, x):
            r = np.sqrt(((X - xi) ** 2).sum(1))
            ref += np.array([qi * 2.0 / (math.sqrt(math.pi) * r_c) if ri < 1e-10 else qi * math.erf(ri / r_c) / ri for ri in r])
        got = f.point_data["Analytical_Solution_atoms"]
        assert f.point_types["Analytical_Solution_atoms"] == ("Float64", 1)
        assert np.abs(got - ref[cd]).max() <= 1e-13 * np.abs(ref).max()
        # GaussianCharges::RightHandSide::value (include/step_50.h:322-329) with libm's exp and pow, as the driver: exact
        den = math.pow(r_c, 3) * math.pow(math.pi, 1.5)
        rhs = np.zeros(len(X))
        for i, xi in enumerate(X):
            s = 0.0
            for d in range(3):
                s += xi[d] * xi[d]
            c = s / (r_c * r_c)
            rhs[i] = (8.0 * math.exp(-4.0 * c) - math.exp(-c)) / den
        assert ore.same_bits(f.point_data["interpolated_rhs"], rhs[cd])
        sup = support_reference(p, inp, origin, h0, 3.5 * r_c)
        for i, s in enumerate(sup):
            got = f.point_data["support_%d" % i]
            assert f.point_types["support_%d" % i] == ("Float32", 1)
            assert got.tobytes() == np.repeat(s, 8).tobytes(), i
        assert 0 < sup[0].sum() < len(sup[0])
    p.close()


def test_optional_arrays_follow_their_keys(tmp_path):
    """each of the reference's three keys alone; the support needs the RHS optimisation"""
    from oracle import gmg_oracle as go

    def arrays(**kw):
        d = tmp_path / ("k%d" % len(os.listdir(tmp_path)))
        p = two_atom_problem(d, cycles=1, **kw)
        p.run_cycle(0, on_device=False)
        h = p.hierarchy()
        p.finish_cycle_with(go.OracleMG(h, smoother=go.SSOR).solve(h.system_rhs)["x"])
        log = p.log()
        p.close()
        return list(ore.read_vtu(os.path.join(d, ore.names(0)[0])).point_data), log

    base = ["solution", "grad_phi", "subdomain", "error_indicator"]
    off = dict(output_analytical=False, output_rhs_field=False, output_atom_support=False)
    assert arrays(**off)[0] == base
    assert arrays(**dict(off, output_analytical=True))[0] == base[:2] + ["Analytical_Solution_atoms"] + base[2:]
    assert arrays(**dict(off, output_rhs_field=True))[0] == base[:2] + ["interpolated_rhs"] + base[2:]
    assert arrays(**dict(off, output_atom_support=True))[0] == base[:2] + ["support_0", "support_1"] + base[2:]
    assert arrays(**dict(off, output_atom_support=True, rhs_optimization=False))[0] == base


def test_analytical_solution_without_lammps_input(tmp_path):
    """GaussianCharges without atoms: Analytical_Solution_without_lammps::value (include/step_50.h:372-376) as is, 0 / 0 at the
    origin included"""
    S = pkg().step50
    p = S.Problem(S.prm_text(left=-1, right=1, mesh_size=0.25, vacuum=1, problem="GaussianCharges", dim=2, bc="Homogeneous", cycles=1, r_c=0.5,
                             global_refinement=0, smoother="SSOR", output_results=True, output_directory=str(tmp_path), output_analytical=True,
                             output_rhs_field=True, output_atom_support=True))
    p.run_cycle(0, on_device=False)
    X = p.dof_coordinates()
    p.finish_cycle_with(np.exp(-8.0 * (X[:, 0] ** 2 + X[:, 1] ** 2)))
    f = ore.read_vtu(os.path.join(tmp_path, ore.names(0)[0]))
    assert list(f.point_data) == ["solution", "grad_phi", "Analytical_Solution_without_lammps", "subdomain", "error_indicator"]   # (the other two need atoms)
    r = np.sqrt(X[:, 0] ** 2 + X[:, 1] ** 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = np.array([(math.erf(2.0 * ri / 0.5) - math.erf(ri / 0.5)) for ri in r]) / (4.0 * math.pi * r)
    cd = np.asarray(p.system_assembly_inputs().cell_dofs).reshape(-1)
    got = f.point_data["Analytical_Solution_without_lammps"]
    assert np.isnan(ref).sum() == 1 and np.array_equal(np.isnan(got), np.isnan(ref[cd]))
    ok = ~np.isnan(ref[cd])
    assert np.abs(got[ok] - ref[cd][ok]).max() <= 1e-13 * np.nanmax(np.abs(ref))
    assert f.types[0] == 9 and f.points[:, 2].tobytes() == np.zeros(f.n_points).tobytes()
    p.close()


def test_more_than_100_atoms_skip_the_supports_with_one_line(tmp_path):
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=3, mesh_size=0.25, vacuum=2, problem="GaussianCharges", dim=3, bc="Homogeneous", cycles=1, r_c=0.5, cutoff=3.5,
                             rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR", output_results=True, output_directory=str(tmp_path),
                             output_analytical=True, output_rhs_field=True, output_atom_support=True))
    p.set_nacl_atoms(3)   # 216 atoms: no analytical solution (10 or more atoms, not on the device), no rhs field, no supports
    p.run_cycle(0, on_device=False)
    X = p.dof_coordinates()
    p.finish_cycle_with(np.sin(X[:, 0]) * np.cos(X[:, 1] + X[:, 2]))
    f = ore.read_vtu(os.path.join(tmp_path, ore.names(0)[0]))
    assert list(f.point_data) == ["solution", "grad_phi", "subdomain", "error_indicator"]
    said = [l for l in p.log().splitlines() if "support of each atom skipped" in l]
    assert said == ["   Output results: support of each atom skipped (216 atoms, at most 100 are written)"]
    p.close()


def test_prm_text_knows_the_keys():
    S = pkg().step50
    text = S.prm_text(output_results=True, output_directory="out", output_analytical=True, output_rhs_field=True, output_atom_support=True)
    for line in ("set Output results = true", "set Output directory = out", "set Output and calculation of Analytical solution = true",
                 "set Output of RHS field = true", "set Output of support of each atom = true"):
        assert line in text
