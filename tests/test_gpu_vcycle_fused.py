"""gmg_precondition with the fused copy_to_mg / copy_from_mg and coarse-level residual against the
sequence they replace: the same bits with every key on and off."""
import copy

import numpy as np
import pytest

from gpu_util import capi, pkg
from oracle import step50_oracle as so

pytestmark = pytest.mark.gpu

KEYS = ("disable_vcycle_fused", "disable_hybrid")
SMOOTHERS = {"Jacobi": 0, "SSOR": 1, "Chebyshev": 2}


@pytest.fixture(scope="module")
def hier_adaptive():
    """8 atoms, adaptive cycles until the hierarchy has three levels: interface matrices, hanging-node rows"""
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous",
                             cycles=6, r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="Jacobi"))
    try:
        p.set_nacl_atoms(1)
        for cycle in range(6):
            if p.run_cycle(cycle, on_device=True)["n_levels"] >= 3:
                break
        h = p.hierarchy()
    finally:
        p.close()
    assert len(h.level_matrices) == 3 and any(m is not None for m in h.edge_matrices)
    return h


def precondition_all_keys(h, kind, seed):
    src = np.random.default_rng(seed).standard_normal(h.system_matrix.n_rows)
    c = capi().Context(len(h.level_matrices))
    try:
        c.load_hierarchy(h)
        c.set_smoother(kind, 0.5, 2, cheb_degree=3)
        vs, vd = c.vector(len(src), src), c.vector(len(src))
        out = {}
        for off in (None,) + KEYS:
            for k in KEYS:
                c.set_option(k, 1 if k == off else 0)
            vd.upload(np.full(len(src), np.nan))
            c.precondition(vd, vs)
            c.precondition(vd, vs)  # (twice: Jacobi swaps the levels' sol <-> w1 buffers between the cycles)
            out[off] = vd.download()
    finally:
        c.close()
    assert np.all(np.isfinite(out[None])) and np.any(out[None] != 0.0)
    for off in KEYS:
        assert np.array_equal(out[off], out[None]), off
    return out[None]


@pytest.mark.parametrize("smoother", sorted(SMOOTHERS))
def test_precondition_equal_with_each_key(hier_adaptive, smoother):
    precondition_all_keys(hier_adaptive, SMOOTHERS[smoother], 11)


def test_dof_on_two_levels_and_levels_without_interface_matrix():
    """Uniform levels (no interface matrices, empty copy lists below the finest), with one system DoF also listed on level 2:
    copy_to_mg fills both rows, copy_from_mg takes the later level of the V-cycle's loop."""
    h = copy.copy(so.build_uniform_hierarchy(3, 0.0, 1.0, 3, problem="Step16"))
    assert all(m is None for m in h.edge_matrices)
    g = h.system_matrix.n_rows // 2 + 3
    row = h.level_matrices[2].n_rows // 2
    h.copy_global, h.copy_level = list(h.copy_global), list(h.copy_level)
    h.copy_global[2] = np.array([g], dtype=np.int32)
    h.copy_level[2] = np.array([row], dtype=np.int32)
    for name, kind in SMOOTHERS.items():
        precondition_all_keys(h, kind, 12)
