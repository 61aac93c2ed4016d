"""Forces on the atoms on the MI355X (gmg_set_point_locator / gmg_atom_forces / gmg_direct_coulomb) against the host mirror
of the same definitions: the field bit for bit, the pair sums to the last bits of erfc / exp."""
import os

import numpy as np
import pytest

from gpu_util import capi, pkg
from test_forces_cpu import affine_field_points, oracle_cycle, problem

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("atoms", ["atom_n1_2.data", "atom_n1_8.data"])
def test_device_field_is_bitwise_the_host_mirror(atoms):
    p = problem(atoms, bc="Inhomogeneous", smoother="Jacobi")
    q, _ = p.atoms()
    for c in range(4):
        rep = p.run_cycle(c, on_device=True)
        phi_d, E_d, F_d = p.atom_forces()  # the cycle ran on the device: the device path
        phi_h, E_h, F_h = p.atom_forces(on_device=False)
        assert np.array_equal(phi_d, phi_h) and np.array_equal(E_d, E_h), c
        fe = 0.0
        for i in range(len(q)):
            fe += 0.5 * q[i] * phi_d[i]
        assert fe == rep["energy_fe_long"], (c, fe, rep["energy_fe_long"])
        assert rel(F_d, F_h) <= 1e-13


def test_linear_reproduction_on_device():
    p = problem("atom_n1_2.data")
    for c in range(3):
        oracle_cycle(p, c)
    p.run_cycle(3, on_device=False)
    a, b = np.array([0.7, -1.3, 0.4]), 0.25
    p.finish_cycle_with(p.dof_coordinates() @ a + b)
    pts = affine_field_points(p)
    p.set_atoms(np.ones(len(pts)), pts)
    phi_d, E_d, _ = p.atom_forces(on_device=True, cutoff=6)
    phi_h, E_h, _ = p.atom_forces(on_device=False, cutoff=6)
    assert np.array_equal(E_d, E_h) and np.array_equal(phi_d, phi_h)
    assert np.abs(E_d + a).max() <= 1e-13 * np.abs(a).max()


@pytest.fixture(scope="module")
def nacl216():
    p = problem("atom_n3_216.data", right=3, cycles=1, bc="Inhomogeneous", smoother="Jacobi")
    p.run_cycle(0, on_device=True)
    return p


@pytest.mark.parametrize("cutoff", [0, 6])
def test_pair_sums_match_the_host_mirror(nacl216, cutoff):
    p = nacl216
    d = p.atom_forces(on_device=True, cutoff=cutoff, parts=True)
    h = p.atom_forces(on_device=False, cutoff=cutoff, parts=True)
    for k in (2, 3, 4):  # F, F^s, e_short
        assert rel(d[k], h[k]) <= 1e-13, (k, rel(d[k], h[k]))
    Fd_d, ed_d = p.direct_coulomb(on_device=True)
    Fd_h, ed_h = p.direct_coulomb(on_device=False)
    assert rel(Fd_d, Fd_h) <= 1e-13 and rel(ed_d, ed_h) <= 1e-13


def test_results_do_not_depend_on_call_or_workgroup_size(nacl216):
    p = nacl216
    ctx = capi().Context.view(p.gmg_context())
    runs = []
    for block in (64, 64, 256, 128):
        ctx.set_option("force_block", block)
        runs.append([p.atom_forces(on_device=True, cutoff=c, parts=True) for c in (0, 6)] + [p.direct_coulomb(on_device=True)])
    ctx.set_option("force_block", 64)
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            for x, y in zip(a, b):
                assert np.array_equal(x, y)


def test_nacl_8000_direct_sum_and_force_error():
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=10.0, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous",
                             cycles=1, r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR",
                             short_range_cutoff=6, compute_forces=True, direct_coulomb_check=True))
    p.set_nacl_atoms(10)
    rep = p.run_cycle(0, on_device=True)
    assert rep["has_forces"]
    Fd_d, ed_d = p.direct_coulomb(on_device=True)
    Fd_h, ed_h = p.direct_coulomb(on_device=False)
    assert rel(Fd_d, Fd_h) <= 1e-12 and rel(ed_d, ed_h) <= 1e-12
    _, _, F_h = p.atom_forces(on_device=False)
    err_h = float(np.sqrt(((F_h - Fd_h) ** 2).sum() / (Fd_h ** 2).sum()))
    assert abs(rep["force_rel_error"] - err_h) <= 1e-9 * err_h, (rep["force_rel_error"], err_h)


def test_invalid_locator_input_is_refused():
    C = capi()
    ctx = C.Context(1)
    try:
        u = ctx.vector(27, np.zeros(27))
        xyz, q = np.array([[0.5, 0.5, 0.5]]), np.array([1.0])
        with pytest.raises(C.GMGError) as e:  # before any locator
            ctx.atom_forces(xyz, q, u, 0.5)
        assert e.value.code == C.ERR_INVALID
        # 2 x 1 x 1 roots, the first split: nodes 0, 1 roots, 2..9 children
        dofs = np.arange(8 * 9, dtype=np.int32).reshape(9, 8) % 27
        node = np.array([2, -1] + [-(k + 2) for k in range(8)], dtype=np.int32)
        for bad in (np.array([9, -1] + list(node[2:]), dtype=np.int32),    # children beyond the end
                    np.array([0, -1] + list(node[2:]), dtype=np.int32),    # a node that is its own child
                    np.array([2, -11] + list(node[2:]), dtype=np.int32)):  # active cell out of range
            with pytest.raises(C.GMGError) as e:
                ctx.set_point_locator([2, 1, 1], [0, 0, 0], 1.0, bad, dofs)
            assert e.value.code == C.ERR_INVALID
        ctx.set_point_locator([2, 1, 1], [0, 0, 0], 1.0, node, dofs)
        out = ctx.atom_forces(xyz, q, u, 0.5)
        assert np.array_equal(out["field"], np.zeros((1, 3)))
        short = ctx.vector(26, np.zeros(26))
        with pytest.raises(C.GMGError) as e:  # a DoF of the locator beyond the end of u
            ctx.atom_forces(xyz, q, short, 0.5)
        assert e.value.code == C.ERR_INVALID
    finally:
        ctx.close()
