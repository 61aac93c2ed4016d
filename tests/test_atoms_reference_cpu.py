"""The host mirror of the atom-side kernels (csrc/gmg_forces.hpp, csrc/gmg_exact.hpp compiled by g++) against the independent
references of tests/atoms_reference.py, no GPU: the same generators, references and bounds as
tests/test_gpu_atoms_reference.py, so that the references and the conditions on the inputs are validated before anything
reaches a device, and the shared text is pinned on the CPU as well.  Each test prints its worst error / bound."""
import functools

import numpy as np
import pytest

import atoms_reference as ar
from test_forces_cpu import problem


@functools.lru_cache(maxsize=None)
def host(r_c):
    """a cycle-0 mesh with a solution (0 but for the boundary values): atom_forces needs one; the atoms are replaced per case"""
    p = problem("atom_n1_2.data", cycles=1, r_c=r_c, quad_rhs=1, smoother="Jacobi")
    p.run_cycle(0, on_device=False)
    p.finish_cycle_with(np.zeros(p.n_dofs()))
    return p


@pytest.mark.parametrize("case_id", list(ar.PAIR_CASES))
def test_short_range_pair_sums(case_id):
    R = ar.pair_reference(case_id)
    ar.check_pair_inputs(case_id, R)
    p = host(R["r_c"])
    p.set_atoms(R["q"], R["x"])
    phi, E, F, Fs, es = p.atom_forces(on_device=False, cutoff=R["cutoff"], parts=True)
    assert np.array_equal(F, R["q"][:, None] * E + Fs)  # F = q E + F^s as formed (E: the boundary values' field, not tested here)
    ar.check_pair_outputs("host mirror", case_id, R, Fs, es)


@pytest.mark.parametrize("case_id", list(ar.DIRECT_CASES))
def test_direct_coulomb(case_id):
    R = ar.pair_reference(case_id, law="direct")
    p = host(0.5)
    p.set_atoms(R["q"], R["x"])
    Fd, ed = p.direct_coulomb(on_device=False)
    ar.check_pair_outputs("host mirror direct", case_id, R, Fd, ed)


@pytest.mark.parametrize("key", list(ar.POTENTIAL_CASES))
def test_exact_potential(key):
    R = ar.potential_reference(key)
    p = host(R["r_c"])
    p.set_atoms(R["q"], R["x"])
    phi, grad = p.gaussian_potential(R["pts"], on_device=False, grad=True)
    ar.check_potential_outputs("host mirror", key, R, phi, grad)
    assert np.array_equal(p.gaussian_potential(R["pts"], on_device=False), phi)


@pytest.mark.parametrize("r_c", [0.5, 0.37])
@pytest.mark.parametrize("n_atoms", [1, 2])
def test_gradient_close_to_an_atom(r_c, n_atoms):
    """Item 4 of the issue: at 2e-10 ... 0.1 r_c from an atom the atom's own contribution to grad phi must be accurate to a
    few ulp of itself (the bound with C = 24 on |q g(s)| / r_c^2), not of the two terms of the closed form, which cancel.
    The closed form alone fails this: it is off by 1.3e-9 of the contribution at 1e-4 r_c and by 0.65 at 1e-8 r_c, and the
    contribution was dropped below r = 1e-10."""
    x, q, pts = ar.near_atom_case(r_c)
    x, q = x[:n_atoms], q[:n_atoms]
    p = host(r_c)
    p.set_atoms(q, x)
    phi, grad = p.gaussian_potential(pts, on_device=False, grad=True)
    ar.check_near_atom("host mirror", r_c, x, q, pts, phi, grad)


def test_reference_tiers_of_the_error_norm_and_the_field_agree():
    """the numpy tiers that the GPU tests apply to all outputs, against mpmath on a sample"""
    rng = np.random.default_rng(9)
    E = ar.error_norm_case()
    for n1 in (1, 2, 3):
        ref = ar.error_norm_reference(E, n1, sample=np.array([0, 1, 30, len(E["h"]) - 1]))
        assert ar.ratio(ref["cell_err2"][ref["sample"]] - ref["mp"], ref["bound_mp"]) <= 1.0 and np.all(ref["cell_err2"] > 0.0)
    A = ar.Forest(6, (4, 4, 4), (-1.3, -1.7, -1.1), 0.5)
    assert set(A.cell_level) == {0, 1, 2, 3, 4}
    pts = ar.forest_points(A, 10, n_random=100, n_special=150)
    u = rng.normal(size=8 * A.n_active)
    f = ar.field_numpy(A, u, pts)
    assert set(f["used"]) >= {0, 1, 2, 4, 8}  # outside, boundary vertex / edge / face, interior
    idx = np.arange(0, len(pts), 9)
    m = ar.field_mp(A, u, pts, idx)
    assert ar.ratio(f["phi"][idx] - m["phi"], f["bound_phi"][idx]) <= 1.0
    assert ar.ratio(f["E"][idx] - m["E"], f["bound_E"][idx]) <= 1.0
    assert np.all(f["E"][f["used"] == 0] == 0.0)
