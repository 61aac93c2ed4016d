"""Forces on the atoms by the host mirror (no GPU): the field of the FE potential at the atoms, the short-range pair
forces of the erfc split and the exact all-pairs Coulomb sum, against numpy restatements of their
definitions, finite differences, and the direct sum."""
import os

import numpy as np
import pytest

from gpu_util import pkg
from oracle import gmg_oracle as go

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def problem(atoms, right=1, cycles=4, **kw):
    S = pkg().step50
    pkg().build.build_all()
    args = dict(left=0, right=right, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Exact", cycles=cycles, r_c=0.5,
                cutoff=3.5, rhs_optimization=True, quad_rhs=4, global_refinement=0, smoother="SSOR")
    args.update(kw)
    p = S.Problem(S.prm_text(**args))
    p.read_lammps(os.path.join(GOLDEN, atoms))
    return p


def oracle_cycle(p, cycle):
    p.run_cycle(cycle, on_device=False)
    h = p.hierarchy()
    r = go.OracleMG(h, smoother=go.SSOR).solve(h.system_rhs, x0=p.vector("initial_guess"))
    assert r["status"] == go.OK
    return p.finish_cycle_with(r["x"])


def affine_field_points(p):
    """Points inside the refined region: DoF positions (vertices, hanging ones on faces and edges of coarser cells), midpoints
    of neighbouring vertices (faces, edges) and random points."""
    X = p.dof_coordinates()
    inner = X[np.all((X > -0.5) & (X < 1.5), axis=1)]
    rng = np.random.default_rng(3)
    pick = inner[rng.choice(len(inner), 400, replace=False)]
    mid = 0.5 * (pick[:200] + pick[200:])
    return np.vstack([pick, mid, rng.uniform(-1.0, 2.0, (200, 3))])


def test_linear_reproduction_on_adaptive_mesh():
    p = problem("atom_n1_2.data")
    for c in range(3):
        oracle_cycle(p, c)
    p.run_cycle(3, on_device=False)
    X = p.dof_coordinates()
    hanging = p.constrained_mask() & np.all((X > -4.9) & (X < 5.9), axis=1)  # constrained, not on the boundary of [-5, 6]^3
    assert p.n_levels() >= 3 and hanging.sum() > 100
    a, b = np.array([0.7, -1.3, 0.4]), 0.25
    u = p.dof_coordinates() @ a + b
    p.finish_cycle_with(u)  # distribute_constraints interpolates the hanging DoFs: u stays affine inside the domain
    pts = affine_field_points(p)
    p.set_atoms(np.ones(len(pts)), pts)
    phi, E, _ = p.atom_forces(on_device=False, cutoff=6)
    assert np.abs(E + a).max() <= 1e-13 * np.abs(a).max(), np.abs(E + a).max()
    assert np.abs(phi - (pts @ a + b)).max() <= 1e-13 * np.abs(pts @ a + b).max()


def erfc_np(v):
    from math import erfc

    return np.vectorize(erfc)(v)


def pair_reference(x, q, r_c, rcut=np.inf):
    d = x[:, None, :] - x[None, :, :]
    r = np.sqrt((d ** 2).sum(-1))
    np.fill_diagonal(r, np.inf)
    qq = q[:, None] * q[None, :]
    mask = r < rcut
    rs = np.where(mask, r, 1.0)
    ec = erfc_np(rs / r_c)
    f = np.where(mask, qq * (ec / rs ** 2 + 2.0 / (np.sqrt(np.pi) * r_c) * np.exp(-rs ** 2 / r_c ** 2) / rs) / rs, 0.0)
    Fs = (f[:, :, None] * d).sum(1)
    es = 0.5 * np.where(mask, qq * ec / rs, 0.0).sum(1)
    Fd = (qq[:, :, None] * d / r[:, :, None] ** 3).sum(1)
    ed = 0.5 * (qq / r).sum(1)
    return Fs, es, Fd, ed


@pytest.fixture(scope="module")
def nacl216():
    p = problem("atom_n3_216.data", right=3, cycles=1)
    p.run_cycle(0, on_device=False)
    p.finish_cycle_with(np.zeros(p.n_dofs()))
    return p


@pytest.mark.parametrize("cutoff", [0, 6, 2.5])
def test_short_range_force_matches_numpy(nacl216, cutoff):
    p = nacl216
    q, x = p.atoms()
    _, E, F, Fs, es = p.atom_forces(on_device=False, cutoff=cutoff, parts=True)
    Fs_ref, es_ref, _, _ = pair_reference(x, q, 0.5, cutoff * 0.5 if cutoff else np.inf)
    scale = np.abs(Fs_ref).max()
    assert np.abs(Fs - Fs_ref).max() <= 1e-13 * scale
    assert np.abs(es - es_ref).max() <= 1e-13 * np.abs(es_ref).max()
    assert np.abs(F - (q[:, None] * E + Fs)).max() <= 1e-15 * scale  # F = q E + F^s, as formed
    assert np.abs(Fs.sum(0)).max() <= 1e-12 * scale  # Newton's third law


def test_short_range_force_is_minus_energy_gradient(nacl216):
    p = nacl216
    q, x = p.atoms()
    _, _, _, Fs, _ = p.atom_forces(on_device=False, cutoff=0, parts=True)
    h = 1e-5
    for i, d in ((0, 0), (17, 1), (101, 2), (215, 0)):
        e = []
        for s in (1, -1):
            y = x.copy()
            y[i, d] += s * h
            p.set_atoms(q, y)
            e.append(sum(p.atom_forces(on_device=False, cutoff=0, parts=True)[4]))
        p.set_atoms(q, x)
        fd = -(e[0] - e[1]) / (2 * h)
        assert abs(fd - Fs[i, d]) <= 1e-6 * np.abs(Fs).max(), (i, d, fd, Fs[i, d])


def test_direct_sum_matches_numpy_and_analytical_energy(nacl216):
    p = nacl216
    q, x = p.atoms()
    Fd, ed = p.direct_coulomb(on_device=False)
    _, _, Fd_ref, ed_ref = pair_reference(x, q, 0.5)
    assert np.abs(Fd - Fd_ref).max() <= 1e-12 * np.abs(Fd_ref).max()
    assert np.abs(ed - ed_ref).max() <= 1e-12 * np.abs(ed_ref).max()
    total = 0.0
    for v in ed:  # summed in atom order, as the host does
        total += v
    ana = p.report(-1)["energy_analytical"]
    assert abs(total - ana) <= 1e-13 * abs(ana), (total, ana)


# measured with the host mirror (oracle solutions, Exact BCs): atom_n1_2 1.62e-2 -> 6.19e-3, NaCl 216 7.10e-3 -> 4.85e-3
# over adaptive cycles 0 -> 3; the bounds are twice the last values
@pytest.mark.parametrize("atoms,right,bound", [("atom_n1_2.data", 1, 1.24e-2), ("atom_n3_216.data", 3, 9.7e-3)])
def test_force_error_against_direct_sum_decreases(atoms, right, bound):
    p = problem(atoms, right=right, compute_forces=True, direct_coulomb_check=True)
    q, _ = p.atoms()
    errs = []
    for c in range(4):
        rep = oracle_cycle(p, c)
        _, _, F = p.atom_forces()
        Fd, _ = p.direct_coulomb()
        err = float(np.sqrt(((F - Fd) ** 2).sum() / (Fd ** 2).sum()))
        assert rep["has_forces"] and abs(rep["force_rel_error"] - err) <= 1e-12 * err
        assert rep["force_max"] == pytest.approx(np.sqrt((F ** 2).sum(1)).max(), rel=1e-15)
        assert np.allclose(rep["force_net"], F.sum(0), rtol=0, atol=1e-13 * np.abs(F).max() * len(q))
        errs.append(err)
    assert errs[-1] < errs[0], errs
    assert errs[-1] < bound, errs


def run_log(**kw):
    p = problem("atom_n1_2.data", cycles=2, **kw)
    for c in range(2):
        oracle_cycle(p, c)
    return p.log()


def test_keys_off_leave_the_log_unchanged():
    plain = run_log()
    assert run_log(compute_forces=False, direct_coulomb_check=False) == plain
    assert "force" not in plain
    on = run_log(compute_forces=True, direct_coulomb_check=True).splitlines()
    extra = [l for l in on if "force" in l]
    assert len(extra) == 6 and [l for l in on if "force" not in l] == plain.splitlines()
    assert extra[0].startswith("Net force on the atoms : (") and extra[1].startswith("Largest force on an atom :")
    assert extra[2].startswith("Relative RMS error of the forces against the direct Coulomb sum :")
