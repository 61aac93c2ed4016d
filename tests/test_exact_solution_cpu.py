"""The exact free-space potential of the Gaussian charges in batches (csrc/gmg_exact.hpp) by its host
mirror, no GPU: the boundary values of `Boundary conditions selection = Exact` and the error in the energy norm with
`Analytical solution on device = true`, against the legacy per-DoF / per-cell host loops and against the numbers the
reference printed."""
import math
import os

import numpy as np

from conftest import rel_close
from gpu_util import pkg
from oracle import gmg_oracle as go
from test_adaptive_golden import check_cycle
from test_forces_cpu import oracle_cycle, problem


def test_host_mirror_equals_the_legacy_host_functions():
    for atoms in ("atom_n1_2.data", "atom_n1_8.data"):
        legacy, mirror = problem(atoms), problem(atoms, analytical_on_device=True)
        for c in range(4):
            a, b = oracle_cycle(legacy, c), oracle_cycle(mirror, c)
            ga, gb = legacy.constraint_inhomogeneities(), mirror.constraint_inhomogeneities()
            assert np.abs(ga).max() > 0.0 and np.array_equal(ga, gb), (atoms, c)
            assert a["cg_iterations"] == b["cg_iterations"]
            ea, eb = a["energy_norm_error"], b["energy_norm_error"]
            print(atoms, c, ea, eb, abs(ea - eb) / ea)
            assert ea > 0 and abs(ea - eb) <= 1e-12 * ea, (atoms, c, ea, eb)
            ce, err = mirror.cell_errors(on_device=False, norm=True)
            assert err == eb and len(ce) == b["active_cells"] and ce.min() >= 0.0
            assert abs(ce.sum() - err ** 2) <= 1e-12 * err ** 2


def test_six_golden_cycles_with_the_key_on(golden, golden_dir):
    """tests/test_adaptive_golden.py's host + oracle run with the boundary values and the error norm through the mirror."""
    G = golden["tests/gaussian-charges.mpirun=1"]["runs"][0]["cycles"]
    S = pkg().step50
    pkg().build.build_all()
    p = S.Problem(S.prm_text(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Exact", cycles=6, r_c=0.5,
                             cutoff=3.5, rhs_optimization=True, quad_rhs=4, global_refinement=0, smoother="SSOR", partition_level0="always",
                             analytical_on_device=True))
    p.read_lammps(os.path.join(golden_dir, "atom_n1_2.data"))
    reps = []
    for cycle in range(6):
        p.run_cycle(cycle, on_device=False)
        h = p.hierarchy()
        b = h.system_rhs
        r = go.OracleMG(h, smoother=go.SSOR).solve(b, x0=p.vector("initial_guess"))
        assert r["status"] == go.OK
        x = r["x"]
        rep = p.finish_cycle_with(x)
        rep.update(cg_iterations=r["iterations"], starting_value=r["starting_value"], convergence_value=r["convergence_value"],
                   sol_l1=float(np.abs(x).sum()), sol_l2=float(np.sqrt(x @ x)), sol_linf=float(np.abs(x).max()))
        g = G[cycle]
        assert rel_close(float(np.abs(b).sum()), g["rhs_l1"], 11) and rel_close(float(np.sqrt(b @ b)), g["rhs_l2"], 11)
        assert rel_close(rep["energy_norm_error"], g["energy_norm_error"], 11), (cycle, rep["energy_norm_error"], g["energy_norm_error"])
        reps.append(rep)
    assert [r["cg_iterations"] for r in reps] == [1, 6, 7, 6, 7, 7]
    assert rel_close(reps[0]["energy_norm_error"], 4.3642174593e-01, 11) and rel_close(reps[5]["energy_norm_error"], 2.3571188349e-01, 11)
    for r, g in zip(reps, G):
        check_cycle(r, g)


def numpy_potential(q, x, r_c, pts):
    """phi and grad restated with math.erf; pairs closer than 1e-10 take the limit value; the gradient's factor is the closed
    form from s = r / r_c = 0.25 on, below it the series of DESIGN.md section 10, and nothing at r = 0"""
    erf = np.vectorize(math.erf)
    d = pts[:, None, :] - x[None, :, :]
    r = np.sqrt((d ** 2).sum(-1))
    near = r < 1e-10
    rs = np.where(near, 1.0, r)
    inv = 1.0 / (math.sqrt(math.pi) * r_c)
    phi = np.where(near, q * 2.0 * inv, q * erf(rs / r_c) / rs).sum(1)
    rs = np.where(r == 0.0, 1.0, r)
    s = rs / r_c
    series = 2.0 / math.sqrt(math.pi) * sum((-1) ** k * 2 * k / ((2 * k + 1) * math.factorial(k)) * s ** (2 * k - 1) for k in range(1, 11))
    closed = (2.0 * rs * np.exp(-s ** 2) * inv - erf(s)) / rs ** 2
    f = np.where(r == 0.0, 0.0, q * np.where(s < 0.25, series / r_c ** 2, closed))
    return phi, (f[:, :, None] * d / rs[:, :, None]).sum(1)


def test_point_on_an_atom_and_numpy_restatement():
    p = problem("atom_n1_8.data", analytical_on_device=True)
    q, x = p.atoms()
    rng = np.random.default_rng(7)
    pts = np.vstack([x[3:4], x[5:6] + 1e-12, rng.uniform(-5.0, 6.0, (200, 3)), x + 0.05])
    phi, grad = p.gaussian_potential(pts, on_device=False, grad=True)
    ref_phi, ref_grad = numpy_potential(q, x, 0.5, pts)
    assert np.isfinite(phi).all() and np.isfinite(grad).all()
    assert np.abs(phi - ref_phi).max() <= 1e-13 * np.abs(ref_phi).max()
    assert np.abs(grad - ref_grad).max() <= 1e-13 * np.abs(ref_grad).max()
    # the point on atom 3: 2 q / (sqrt(pi) r_c) plus the other atoms, which the reference formula covers
    others = np.arange(len(q)) != 3
    rest, _ = numpy_potential(q[others], x[others], 0.5, pts[:1])
    assert abs(phi[0] - (2.0 * q[3] / (math.sqrt(math.pi) * 0.5) + rest[0])) <= 1e-14 * abs(phi).max()
    assert np.array_equal(p.gaussian_potential(pts, on_device=False), phi)  # phi alone: the same sums


def test_keys_off_by_default_and_the_large_system_gate():
    S = pkg().step50
    kw = dict(left=0, right=2.0, mesh_size=0.5, vacuum=2, problem="GaussianCharges", dim=3, bc="Exact", cycles=1, r_c=0.5, cutoff=3.5,
              rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="Jacobi")

    def log(**extra):  # 512 atoms: beyond the reference's 300-atom gate
        p = S.Problem(S.prm_text(**kw, **extra))
        p.set_nacl_atoms(4)
        p.run_cycle(0, on_device=False)
        rep = p.finish_cycle_with(np.zeros(p.n_dofs()))
        return p.log(), rep

    plain, _ = log()
    one, _ = log(analytical_on_device=True)
    assert "energy norm" not in plain and one == plain  # the first key alone prints what the legacy run prints
    assert log(error_norm_for_large_systems=True)[0] == plain  # the second key alone lifts nothing
    both, rep = log(analytical_on_device=True, error_norm_for_large_systems=True)
    lines = both.splitlines()
    extra = [l for l in lines if "energy norm" in l]
    assert len(extra) == 1 and extra[0].startswith("Error in FE solution in energy norm:  ")
    assert [l for l in lines if "energy norm" not in l] == plain.splitlines()
    assert rep["energy_norm_error"] > 0.0 and float(extra[0].split()[-1]) == float("%.10e" % rep["energy_norm_error"])
