"""Device memory over whole life cycles of a context (csrc/gmg_mem.hpp: every allocation of the library has one owner whose
destructor frees it): the free memory of the device after N rounds of create / set up / solve / forces / reset / set up
again / destroy equals the free memory after the first round, and the same for rounds of calls the library refuses with an
error code.  The first round absorbs what the runtime allocates once per process (code objects, queues, its own pools)."""
import numpy as np
import pytest

import rhs_reference as rr
from gpu_util import capi, pkg

pytestmark = pytest.mark.gpu

ROUNDS = 6


def free_bytes():
    import torch

    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def free_after_rounds(one_round):
    free = []
    for _ in range(ROUNDS):
        one_round()
        free.append(free_bytes())
    print("free device memory after each round, relative to the first:", [f - free[0] for f in free])
    return free


def test_no_leak_across_life_cycles():
    """the small problem of smoke() (8 atoms, 45^3 lattice), everything on the device: cycle 0 creates the context, computes
    the charge densities (gmg_charge_density), sets the hierarchy up, assembles the right-hand side (gmg_rhs_assemble) and
    solves; the forces set the point locator (gmg_set_point_locator, gmg_atom_forces); cycle 1 refines, which resets the
    context (gmg_reset), builds the transfer between its two levels on the device (gmg_build_transfer), sets up again and
    solves; close() destroys the context.  Condition: equality of the free memory after round 1 and after round N."""
    S = pkg().step50

    def one_round():
        p = S.Problem(S.prm_text(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=2,
                                 r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR",
                                 densities_on_device=True, rhs_on_device=True, transfer_on_device=True, short_range_cutoff=6))
        try:
            p.set_nacl_atoms(1)
            rep = p.run_cycle(0, on_device=True)
            assert rep["cg_iterations"] >= 1
            _, _, F = p.atom_forces(on_device=True)
            assert np.isfinite(F).all()
            rep = p.run_cycle(1, on_device=True)
            assert rep["cg_iterations"] >= 1 and p.n_levels() >= 2
            _, _, F = p.atom_forces(on_device=True)
            assert np.isfinite(F).all()
        finally:
            p.close()

    free = free_after_rounds(one_round)
    assert free[-1] == free[0], free


def test_no_leak_across_refused_calls():
    """calls that are refused with GMG_ERR_INVALID after their validation has started (the refusals of
    test_gpu_rhs_reference.py and test_gpu_forces.py), each followed by the call that works, in a context of its own per round"""
    C = capi()
    T = rr.rhs_tables("d3-nq8")
    G = T["geometry"]
    n_dofs = len(T["dof_ptr"]) - 1
    dofs = np.arange(8 * 9, dtype=np.int32).reshape(9, 8) % 27
    node = np.array([2, -1] + [-(k + 2) for k in range(8)], dtype=np.int32)
    xyz, q = np.array([[0.5, 0.5, 0.5]]), np.array([1.0])

    def assemble(c, tables):
        out = c.vector(n_dofs)
        try:
            c.rhs_assemble(tables["n_cells"], tables["dim"], tables["shape"], tables["weight"], tables["cell_level"], tables["jxw"],
                           tables["term_slot"], tables["term_value"], tables["dof_ptr"], tables["entry_slot"], tables["entry_coef"],
                           tables["coef_table"], out)
        finally:
            out.free()

    def refused(call):
        with pytest.raises(C.GMGError) as e:
            call()
        assert e.value.code == C.ERR_INVALID

    def one_round():
        c = C.Context(1)
        try:
            refused(lambda: assemble(c, T))  # no densities on the device yet
            c.charge_density(G["cell_lo"], G["cell_h"], G["root_lo"], G["root_h"], G["x"], G["q"], G["r_c"], G["cutoff"], False, G["qp"], dens=None)
            refused(lambda: c.get_charge_density(T["n_cells"] + 1, T["nq"]))
            ptr = T["dof_ptr"].copy()
            ptr[7] = ptr[6] - 1  # not monotone
            refused(lambda: assemble(c, dict(T, dof_ptr=ptr)))
            es = T["entry_slot"].copy()
            es[5] = T["n_cells"] * 8  # slot out of range
            refused(lambda: assemble(c, dict(T, entry_slot=es)))
            assemble(c, T)
            u = c.vector(27, np.zeros(27))
            short = c.vector(26, np.zeros(26))
            refused(lambda: c.atom_forces(xyz, q, u, 0.5))  # before any locator
            for bad in ([9, -1], [0, -1], [2, -11]):  # children beyond the end, a node that is its own child, cell out of range
                refused(lambda: c.set_point_locator([2, 1, 1], [0, 0, 0], 1.0, np.array(bad + list(node[2:]), dtype=np.int32), dofs))
            c.set_point_locator([2, 1, 1], [0, 0, 0], 1.0, node, dofs)
            refused(lambda: c.atom_forces(xyz, q, short, 0.5))  # a DoF of the locator beyond the end of u
            refused(lambda: c.set_point_locator([2, 1, 1], [0, 0, 0], 1.0, np.array([9, -1] + list(node[2:]), dtype=np.int32), dofs))
            refused(lambda: c.atom_forces(xyz, q, u, 0.5))  # the refused call dropped the locator
            c.set_point_locator([2, 1, 1], [0, 0, 0], 1.0, node, dofs)
            c.atom_forces(xyz, q, u, 0.5)
            u.free()
            short.free()
        finally:
            c.close()

    free = free_after_rounds(one_round)
    assert free[-1] == free[0], free
