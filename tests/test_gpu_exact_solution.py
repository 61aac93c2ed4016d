"""The exact free-space potential of the Gaussian charges on the MI355X (gmg_gaussian_potential / gmg_energy_norm_error,
prm keys `Analytical solution on device` and `Error norm for large systems`) against the host mirror
of the same text (csrc/gmg_exact.hpp): sums that differ only by erf / exp / sqrt of the two math libraries."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import rel_close
from gpu_util import capi, pkg
from test_adaptive_golden import KEYS11, check_cycle
from test_exact_solution_cpu import numpy_potential
from test_forces_cpu import problem

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def nacl1000(cycles=2, **kw):
    return problem("atom_n5_1000.data", right=5, cycles=cycles, quad_rhs=1, **kw)


def sample_points(x):
    """lattice nodes (those on multiples of 2.5 sit on atoms), random points, one more atom position"""
    g = np.arange(-5.0, 10.0 + 1e-9, 1.25)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(11)
    return np.vstack([lattice, rng.uniform(-5.0, 10.0, (2000, 3)), x[417:418]])


def test_potential_matches_host_mirror_and_numpy():
    p = nacl1000()
    q, x = p.atoms()
    assert len(q) == 1000
    pts = sample_points(x)
    ctx = capi().Context(1)
    try:
        phi_d, grad_d = ctx.gaussian_potential(x, q, 0.5, pts)
        only_phi, none = ctx.gaussian_potential(x, q, 0.5, pts, want_grad=False)
        none2, only_grad = ctx.gaussian_potential(x, q, 0.5, pts, want_phi=False)
    finally:
        ctx.close()
    assert none is None and none2 is None and np.array_equal(only_phi, phi_d) and np.array_equal(only_grad, grad_d)
    phi_h, grad_h = p.gaussian_potential(pts, on_device=False, grad=True)
    print("device vs host mirror:", rel(phi_d, phi_h), rel(grad_d, grad_h))
    assert np.isfinite(phi_d).all() and np.isfinite(grad_d).all()
    assert rel(phi_d, phi_h) <= 1e-13 and rel(grad_d, grad_h) <= 1e-13
    phi_n, grad_n = numpy_potential(q, x, 0.5, pts)
    print("device vs numpy:", rel(phi_d, phi_n), rel(grad_d, grad_n))
    assert rel(phi_d, phi_n) <= 1e-12 and rel(grad_d, grad_n) <= 1e-12


def test_bits_do_not_depend_on_workgroup_size_chunks_or_call():
    p = nacl1000()
    q, x = p.atoms()
    pts = sample_points(x)
    ctx = capi().Context(1)
    try:
        runs = []
        for block, chunk in ((64, 35), (64, 35), (128, 35), (256, 35), (64, 13), (256, 17), (128, 0)):
            ctx.set_option("force_block", block)
            ctx.set_option("exact_chunk_log2", chunk)  # 2^13 / 1000 atoms: 8 points per launch; 0: one point per launch
            runs.append(ctx.gaussian_potential(x, q, 0.5, pts if chunk else pts[-300:]))
        with pytest.raises(capi().GMGError):
            ctx.set_option("exact_chunk_log2", 36)
    finally:
        ctx.close()
    for phi, grad in runs[1:-1]:
        assert np.array_equal(phi, runs[0][0]) and np.array_equal(grad, runs[0][1])
    assert np.array_equal(runs[-1][0], runs[0][0][-300:]) and np.array_equal(runs[-1][1], runs[0][1][-300:])


def test_six_golden_cycles_on_device_with_the_key_on(golden, golden_dir):
    G = golden["tests/gaussian-charges.mpirun=1"]["runs"][0]["cycles"]
    S = pkg().step50
    pkg().build.build_all()

    def make():
        p = S.Problem(S.prm_text(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Exact", cycles=6,
                                 r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=4, global_refinement=0, smoother="SSOR",
                                 partition_level0="always", analytical_on_device=True))
        p.read_lammps(os.path.join(golden_dir, "atom_n1_2.data"))
        return p

    dev, host = make(), make()
    reps = []
    for c in range(6):
        r = dev.run_cycle(c, on_device=True)
        host.run_cycle(c, on_device=False)  # the same mesh: it refines on the device's solution
        host.finish_cycle_with(dev.vector("solution"))
        gd, gh = dev.constraint_inhomogeneities(), host.constraint_inhomogeneities()
        print(c, "boundary values device vs host mirror:", rel(gd, gh), "error norm", r["energy_norm_error"])
        assert rel(gd, gh) <= 1e-13, (c, rel(gd, gh))
        b = dev.vector("rhs")
        assert rel_close(float(np.abs(b).sum()), G[c]["rhs_l1"], 11) and rel_close(float(np.sqrt(b @ b)), G[c]["rhs_l2"], 11)
        assert rel_close(r["energy_norm_error"], G[c]["energy_norm_error"], 11), (c, r["energy_norm_error"])
        reps.append(r)
    assert [r["cg_iterations"] for r in reps] == [1, 6, 7, 6, 7, 7]
    assert rel_close(reps[0]["energy_norm_error"], 4.3642174593e-01, 11) and rel_close(reps[5]["energy_norm_error"], 2.3571188349e-01, 11)
    for r, g in zip(reps, G):
        check_cycle(r, g)
        for k in KEYS11:
            assert rel_close(r[k], g[k], 11), k
        assert rel_close(r["matrix_frobenius"], g["matrix_frobenius"], 10)


def test_error_norm_of_1000_atoms_on_device():
    """1000 atoms are beyond the reference's 300-atom gate: both keys on."""
    on = nacl1000(analytical_on_device=True, error_norm_for_large_systems=True)
    off = nacl1000()
    for c in range(2):
        r, r_off = on.run_cycle(c, on_device=True), off.run_cycle(c, on_device=True)
        assert (r["cg_iterations"], r["coarse_iterations"]) == (r_off["cg_iterations"], r_off["coarse_iterations"])
        assert r["active_cells"] == r_off["active_cells"] and r_off["energy_norm_error"] == 0.0
        assert rel(on.constraint_inhomogeneities(), off.constraint_inhomogeneities()) <= 1e-13
        ce_d, err_d = on.cell_errors(norm=True)  # the cycle ran on the device: the device path
        ce_h, err_h = on.cell_errors(on_device=False, norm=True)
        print(c, "cells", len(ce_d), "error norm device / host mirror:", r["energy_norm_error"], err_h, "cells:", rel(ce_d, ce_h))
        assert r["energy_norm_error"] == err_d and err_h > 0.0
        assert abs(err_d - err_h) <= 1e-12 * err_h
        assert len(ce_d) == r["active_cells"] and rel(ce_d, ce_h) <= 1e-12
        assert abs(ce_d.sum() - err_d ** 2) <= 1e-12 * err_d ** 2
        assert sum("Error in FE solution in energy norm" in l for l in on.log().splitlines()) == c + 1
    assert "energy norm" not in off.log()
    # launch shape and chunking change no bit of the error norm either
    ctx = capi().Context.view(on.gmg_context())
    for block, chunk in ((128, 35), (256, 24), (64, 35)):
        ctx.set_option("force_block", block)
        ctx.set_option("exact_chunk_log2", chunk)  # 2^24 / 1000 atoms / 8 points: 2097 cells per launch
        ce, err = on.cell_errors(norm=True)
        assert np.array_equal(ce, ce_d) and err == err_d, (block, chunk)
    # the first key alone: the boundary batch runs, the gate stays
    first = nacl1000(cycles=1, analytical_on_device=True)
    r = first.run_cycle(0, on_device=True)
    assert "energy norm" not in first.log() and r["energy_norm_error"] == 0.0


def test_invalid_input_is_refused_and_empty_calls_pass():
    Cp = capi()
    ctx = Cp.Context(1)
    try:
        x, q, pts = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]]), np.array([1.0, -1.0]), np.array([[0.25, 0.25, 0.25]])
        D = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        out = np.zeros(1)
        for r_c in (0.0, -1.0, float("nan")):
            with pytest.raises(Cp.GMGError) as e:
                ctx.gaussian_potential(x, q, r_c, pts)
            assert e.value.code == Cp.ERR_INVALID
        L = ctx.L
        assert L.gmg_gaussian_potential(ctx.h, C.c_int64(2), D(x), D(q), C.c_double(0.5), C.c_int64(1), None, D(out), None) == Cp.ERR_INVALID
        assert L.gmg_gaussian_potential(ctx.h, C.c_int64(-1), D(x), D(q), C.c_double(0.5), C.c_int64(1), D(pts), D(out), None) == Cp.ERR_INVALID
        assert L.gmg_gaussian_potential(ctx.h, C.c_int64(2), D(x), D(q), C.c_double(0.5), C.c_int64(-1), D(pts), D(out), None) == Cp.ERR_INVALID
        assert L.gmg_gaussian_potential(ctx.h, C.c_int64(2), None, D(q), C.c_double(0.5), C.c_int64(1), D(pts), D(out), None) == Cp.ERR_INVALID
        # empty calls: no points; no atoms (the potential of nothing is 0)
        assert L.gmg_gaussian_potential(ctx.h, C.c_int64(2), D(x), D(q), C.c_double(0.5), C.c_int64(0), None, None, None) == Cp.OK
        phi, grad = ctx.gaussian_potential(np.zeros((0, 3)), np.zeros(0), 0.5, pts)
        assert np.array_equal(phi, [0.0]) and np.array_equal(grad, np.zeros((1, 3)))
        # the error norm: one unit cube, u = x (grad phi_h = e_x), midpoint rule
        lo, hh, dofs = np.zeros((1, 3)), np.ones(1), np.arange(8, dtype=np.int32).reshape(1, 8)
        u = ctx.vector(8, np.array([0.0, 1.0] * 4))
        qp, w = np.array([[0.5, 0.5, 0.5]]), np.array([1.0])
        sg = np.array([[[(1 if (a >> d) & 1 else -1) * 0.25 for d in range(3)] for a in range(8)]])
        err, ce = ctx.energy_norm_error(lo, hh, dofs, u, np.zeros((0, 3)), np.zeros(0), 0.5, qp, w, sg)
        assert err == 1.0 and np.array_equal(ce, [1.0])  # no atoms: || e_x || over the unit cube
        err, ce = ctx.energy_norm_error(np.zeros((0, 3)), np.zeros(0), np.zeros((0, 8), dtype=np.int32), u, x, q, 0.5, qp, w, sg)
        assert err == 0.0 and len(ce) == 0  # no cells
        for bad in (dict(r_c=0.0), dict(dofs=np.array([[0, 1, 2, 3, 4, 5, 6, 8]], dtype=np.int32)),
                    dict(dofs=np.array([[0, 1, 2, 3, 4, 5, 6, -1]], dtype=np.int32))):
            with pytest.raises(Cp.GMGError) as e:
                ctx.energy_norm_error(lo, hh, bad.get("dofs", dofs), u, x, q, bad.get("r_c", 0.5), qp, w, sg)
            assert e.value.code == Cp.ERR_INVALID
        u.free()
    finally:
        ctx.close()
