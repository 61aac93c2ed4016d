"""GPU tests of the whole drop-in path: host C++ (LaplaceProblem mirror) -> C-ABI -> HIP,
against the reference's golden logs and the oracle."""
import os

import numpy as np
import pytest

from conftest import rel_close
from gpu_util import pkg
from oracle import gmg_oracle as go

pytestmark = pytest.mark.gpu


def _problem(**kw):
    S = pkg().step50
    return S.Problem(S.prm_text(**kw))


def test_cycle0_two_atoms_matches_reference_log(golden, golden_dir):
    """tests/gaussian-charges.mpirun=1.output:8-29, all printed quantities incl. energies."""
    g = golden["tests/gaussian-charges.mpirun=1"]["runs"][0]["cycles"][0]
    p = _problem(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Exact", cycles=1,
                 r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=4, global_refinement=0, smoother="SSOR")
    p.read_lammps(os.path.join(golden_dir, "atom_n1_2.data"))
    r = p.run_cycle(0)
    assert r["cg_iterations"] == g["cg_iterations"] == 1 and r["coarse_iterations"] == 112
    for k in ("rhs_l1", "rhs_l2", "rhs_linf", "matrix_l1", "matrix_linf", "matrix_frobenius", "sol_l1", "sol_l2", "sol_linf"):
        assert rel_close(r[k], g[k], 11), k
    assert abs(r["starting_value"] - g["starting_value"]) < 0.6e-10
    assert abs(r["convergence_value"] - g["convergence_value"]) < 1e-5 * g["convergence_value"]
    for k in ("energy_analytical", "energy_short", "energy_fe_long", "energy_self"):
        assert rel_close(r[k], g[k], 11), k
    assert rel_close(r["energy_total"], g["energy_total_split"], 11)
    assert rel_close(r["energy_abs_error"], g["energy_abs_error"], 10)
    log = p.log()
    assert "   CG converged in 1 iterations." in log and "   L1 solution norm 1.2024932115e+03" in log


@pytest.mark.parametrize("device_cg", [False, True])
def test_five_level_jacobi_host_cg_and_device_cg(golden, device_cg):
    g = golden["tests_3D/step-16.mpirun=1"]["runs"][0]["cycles"][0]
    p = _problem(left=0, right=1, problem="Step16", dim=3, bc="Homogeneous", cycles=1, global_refinement=4,
                 smoother="Jacobi", device_cg=device_cg)
    r = p.run_cycle(0)
    assert r["cg_iterations"] == g["cg_iterations"] == 8
    for k in ("sol_l1", "sol_l2", "sol_linf"):
        assert rel_close(r[k], g[k], 6)
    r2 = p.solve_again()
    assert r2["cg_iterations"] == 8


def test_solution_matches_oracle_all_smoothers():
    for sm, kind in (("Jacobi", go.JACOBI), ("Chebyshev", go.CHEBYSHEV), ("SSOR", go.SSOR)):
        p = _problem(left=0, right=1, problem="Step16", dim=3, bc="Homogeneous", cycles=1, global_refinement=4, smoother=sm)
        r = p.run_cycle(0)
        h = p.hierarchy()
        ref = go.OracleMG(h, smoother=kind).solve(h.system_rhs)
        assert r["cg_iterations"] == ref["iterations"], sm
        x = p.vector("solution")
        assert np.abs(x - ref["x"]).max() <= 1e-9 * np.abs(ref["x"]).max(), sm


def test_distributed_layout_on_one_rank(golden):
    """The N > 1 code path (RCCL communicator, partitioned level 0 + system rows, replicated
    upper levels, all-gathers around the V-cycle) with world size 1 must reproduce the golden."""
    g = golden["tests_3D/step-16.mpirun=1"]["runs"][0]["cycles"][0]
    capi = pkg().capi
    p = _problem(left=0, right=1, problem="Step16", dim=3, bc="Homogeneous", cycles=1, global_refinement=4, smoother="Jacobi",
                 partition_level0="always")
    p.set_communicator(0, 1, capi.Context.unique_id())
    r = p.run_cycle(0)
    assert r["cg_iterations"] == g["cg_iterations"] == 8
    for k in ("sol_l1", "sol_l2", "sol_linf"):
        assert rel_close(r[k], g[k], 6)
    p2 = _problem(left=0, right=1, mesh_size=0.25, vacuum=4, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=1,
                  r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="Jacobi",
                  partition_level0="always")
    p2.set_nacl_atoms(1)
    ref = _problem(left=0, right=1, mesh_size=0.25, vacuum=4, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=1,
                   r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="Jacobi")
    ref.set_nacl_atoms(1)
    p2.set_communicator(0, 1, capi.Context.unique_id())
    a, b = p2.run_cycle(0), ref.run_cycle(0)
    assert a["cg_iterations"] == b["cg_iterations"] and a["coarse_iterations"] == b["coarse_iterations"]
    xa, xb = p2.vector("solution"), ref.vector("solution")
    assert np.abs(xa - xb).max() <= 1e-9 * np.abs(xb).max()


def test_charge_density_on_device_matches_host(golden, golden_dir):
    """gmg_charge_density (src/step-50.cc:509-575 + the cutoff lists of :260-306)
    against the host evaluation of the same sums, and against the rhs norms the reference
    printed (tests/gaussian-charges.mpirun=1.output:10-12; QGauss(5): 125 points per cell)."""
    g = golden["tests/gaussian-charges.mpirun=1"]["runs"][0]["cycles"][0]
    rhs = {}
    for dev in (True, False):
        for opt in (True, False):
            p = _problem(left=0, right=1, mesh_size=0.25, vacuum=4 if not opt else 10, problem="GaussianCharges", dim=3, bc="Exact",
                         cycles=1, r_c=0.5, cutoff=3.5, rhs_optimization=opt, quad_rhs=4, global_refinement=0, smoother="Jacobi",
                         densities_on_device=dev)
            p.read_lammps(os.path.join(golden_dir, "atom_n1_2.data"))
            r = p.run_cycle(0)
            rhs[(dev, opt)] = p.vector("rhs")
            if opt:
                for k in ("rhs_l1", "rhs_l2", "rhs_linf"):
                    assert rel_close(r[k], g[k], 11), (dev, k)
    for opt in (True, False):
        a, b = rhs[(True, opt)], rhs[(False, opt)]
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()
    # 216 atoms, lists on: many atoms per cell, bins with several atoms
    out = []
    for dev in (True, False):
        p = _problem(left=0, right=3, mesh_size=0.25, vacuum=2, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=1,
                     r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="Jacobi",
                     densities_on_device=dev)
        p.set_nacl_atoms(3)
        p.run_cycle(0)
        out.append(p.vector("rhs"))
    assert np.abs(out[0] - out[1]).max() <= 1e-13 * np.abs(out[1]).max()


def test_cli_output_diffs_against_reference_output_file(golden_dir, tmp_path):
    """./step50_mi355x file.prm (the counterpart of the reference's ./main, src/main.cc) on the
    parameters of tests/gaussian-charges.cc: every line the reference's expected output
    (tests/gaussian-charges.mpirun=1.output) shares with ours is compared number by number,
    the way deal.II's numdiff-based test harness does."""
    import re
    import subprocess

    exe = pkg().build.EXE_HOST
    prm = tmp_path / "gaussian-charges.prm"
    prm.write_text(pkg().step50.prm_text(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Exact",
                                         cycles=6, r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=4, global_refinement=0,
                                         smoother="SSOR", lammps=os.path.join(golden_dir, "atom_n1_2.data")))
    out = subprocess.run([exe, str(prm)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    num = re.compile(r"(?<![A-Za-z_])[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?")

    def keyed(text):
        d, cycle = {}, None
        for line in text.splitlines():
            line = line.strip()
            m = re.match(r"Cycle (\d+):", line)
            if m:
                cycle = int(m.group(1))
                continue
            label = num.sub("#", line)
            if cycle is not None and num.search(line):
                d.setdefault((cycle, label), [float(x) for x in num.findall(line)])
        return d

    ours = keyed(out.stdout)
    ref = keyed(open(os.path.join(golden_dir, "gaussian-charges.mpirun=1.output")).read())
    shared = [k for k in ref if k in ours]
    assert len(shared) >= 6 * 20  # >= 20 labelled lines in each of the 6 cycles
    for k in shared:
        for a, b in zip(ours[k], ref[k]):
            tol = 2e-5 if "Convergence value" in k[1] else 2e-10
            assert abs(a - b) <= tol * max(abs(b), 1e-300) or abs(a - b) < 1e-12, (k, a, b)
    missing = sorted({k[1] for k in ref if k not in ours})
    assert missing == [], missing


def test_rhs_cutoff_lists_on_device_match_reference_error_table(golden, golden_dir):
    """The same error-versus-cutoff table with the charge densities evaluated by charge_density_kernel."""
    from test_host import check_rc_variation

    check_rc_variation(golden, golden_dir, on_device=True)


def test_short_range_energy_with_cutoff_and_for_large_systems(golden_dir):
    """SURVEY 8(f) N3, second half: the erfc pair sum over the pairs within 6 smoothing lengths (cell bins) equals the
    reference's all-pairs sum (src/step-50.cc:1325-1332) to the last digits on 216 atoms, and lets the energy be evaluated
    for 1000 atoms, which the reference skips (number_of_atoms < 300, :1554)."""
    S = pkg().step50

    def run(nacl, **kw):
        p = S.Problem(S.prm_text(left=0, right=float(nacl), mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=1,
                                 r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="Jacobi", **kw))
        p.set_nacl_atoms(nacl)
        r = p.run_cycle(0, on_device=True)
        p.close()
        return r

    a, b = run(3), run(3, short_range_cutoff=6.0)
    assert a["has_energy"] and b["has_energy"]
    assert abs(a["energy_short"] - b["energy_short"]) <= 1e-13 * abs(a["energy_short"])
    assert abs(a["energy_total"] - b["energy_total"]) <= 1e-13 * abs(a["energy_total"])
    assert a["energy_fe_long"] == b["energy_fe_long"] and a["energy_analytical"] == b["energy_analytical"]
    big = run(5)
    assert not big["has_energy"]  # the reference's gate
    big = run(5, short_range_cutoff=6.0, energy_for_large_systems=True)
    assert big["has_energy"] and np.isfinite(big["energy_total"]) and big["energy_short"] < 0.0
    # NaCl lattice: the short-ranged energy per ion of 1000 atoms is that of 216 atoms up to the surface share (measured: 5.1 %)
    assert abs(big["energy_short"] / 1000 - a["energy_short"] / 216) <= 0.10 * abs(a["energy_short"] / 216)


@pytest.mark.parametrize("device_cg", [False, True])
def test_preconditioner_jacobi_through_the_driver(golden_dir, device_cg):
    """Preconditioner = Jacobi on the device: upload() hands over the system matrix, the vectors and the rhs and no level (the
    levels are not assembled for it), SolverCG_solve (device_cg false) and gmg_cg_solve (true) run gmg_precondition_jacobi.
    Two adaptive cycles with the geometry of case B3 of tests/mg_cases.py, each against tests/cg_reference.py on the cycle's
    own system matrix, rhs and initial guess; tests/test_host.py (test_preconditioner_jacobi_host_cycles) shows that no
    rounding moves the iteration count on these cycles."""
    from test_host import check_jacobi_cycle, jacobi_references, preconditioner_problem

    p = preconditioner_problem(golden_dir, preconditioner="Jacobi", device_cg=device_cg)
    worst = 0.0
    for cycle in range(2):
        rep = p.run_cycle(cycle, on_device=True)
        refs, tol, spread = jacobi_references(p)
        worst = max(worst, check_jacobi_cycle(rep, p.vector("solution"), p, refs, spread))
        assert rep["coarse_iterations"] == 0
        with pytest.raises(RuntimeError):   # (no level matrix exists, on the host or on the device: none is read)
            p.hierarchy()
    p.close()
    print(f"\n[host-gpu] Jacobi through the driver, device_cg {device_cg}: |x - ref| / tolerance max {worst:.3f}")
