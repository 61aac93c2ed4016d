"""gmg_assemble_system_matrix, gmg_get_system_matrix and gmg_system_matrix_norms on the MI355X (csrc/gmg_assemble.hpp)
against the host driver's assembly and the independent restatement of tests/system_matrix_reference.py, bit for bit; the
operator they leave behind against gmg_set_system_matrix with the host CSR; and whole adaptive runs with
"System matrix on device" against the same runs without it."""
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

import system_matrix_reference as smr
from gpu_util import capi, pkg
from test_system_matrix_cpu import MESHES, line_kinds, problem

pytestmark = pytest.mark.gpu

GPU_MESHES = MESHES + [("atom_n5_1000.data", 5.0, 3)]


@pytest.fixture()
def ctx():
    c = capi().Context(1)
    yield c
    c.close()


def assemble(ctx, inp, **kw):
    return ctx.assemble_system_matrix(inp.dim, inp.n_dofs, inp.cell_dofs, inp.cell_level, inp.K_of_level, inp.constraint_of_dof,
                                      inp.line_ptr, inp.line_master, inp.line_weight, **kw)


def frobenius_close(value, host_val):
    """sqrt(fsum(v^2)) within (nnz + 2) 2^-53 relative: the worst case of a sum of nnz non-negative terms in any order
    (each term and each partial sum rounded once) plus the square root"""
    exact = math.sqrt(math.fsum(float(v) * float(v) for v in host_val))
    print(f"frobenius: device {value!r} exact {exact!r} rel {abs(value - exact) / exact:.3e} bound {(len(host_val) + 2) * 2.0 ** -53:.3e}")
    return abs(value - exact) <= (len(host_val) + 2) * 2.0 ** -53 * exact


@pytest.mark.parametrize("name,right,cycles", GPU_MESHES, ids=[m[0] for m in GPU_MESHES])
def test_download_norms_and_operator_equal_the_host(golden_dir, name, right, cycles):
    p = problem(golden_dir, name, right, cycles, system_matrix_on_device=True)
    seen = np.zeros(3, dtype=np.int64)
    for cycle in range(cycles):
        rep = p.run_cycle(cycle, on_device=True)
        assert p.system_matrix_on_device() and "not applicable" not in p.log()
        dev = p.device_system_matrix()
        inp = p.system_assembly_inputs()
        seen += line_kinds(inp)
        host = p.matrix("system")  # assembled on the host now, on demand
        assert smr.same_bits(dev, host), cycle
        assert smr.same_bits(dev, smr.assemble(inp)), cycle
        # the printed norms came from the device
        # (CSRMatrix::l1_norm / linfty_norm restated on the host's arrays)
        col_sum = np.zeros(host.n_rows)
        np.add.at(col_sum, host.col, np.abs(host.val))
        row_sum = np.zeros(host.n_rows)
        np.add.at(row_sum, np.repeat(np.arange(host.n_rows), np.diff(host.rowptr)), np.abs(host.val))
        assert rep["matrix_l1"] == col_sum.max() and rep["matrix_linf"] == row_sum.max(), cycle
        assert frobenius_close(rep["matrix_frobenius"], host.val)
        # launch shape: a second context, one workgroup and then three (every kernel's grid-stride loop iterates) -- the same
        # bits, and the same operator as the host CSR gives
        a, b = capi().Context(1), capi().Context(1)
        for max_blocks in (1, 3):
            a.set_option("assemble_max_blocks", max_blocks)
            assemble(a, inp)
            assert smr.same_bits(a.get_system_matrix(), dev), (cycle, max_blocks)
            assert a.system_matrix_norms()[:2] == (rep["matrix_l1"], rep["matrix_linf"]), (cycle, max_blocks)
        b.set_system_matrix(host)
        x = np.cos(np.arange(host.n_rows) * 0.37) + 0.25
        for c in (a, b):
            c.x, c.y, c.z = c.vector(host.n_rows, x), c.vector(host.n_rows), c.vector(host.n_rows)
            c.spmv(capi().SYSTEM, c.y, c.x)
            c.precondition_jacobi(0.6, c.z, c.x)
        for u, v in ((a.y, b.y), (a.z, b.z)):
            assert np.array_equal(u.download().view(np.uint64), v.download().view(np.uint64)), cycle
        a.close()
        b.close()
    assert seen[0] > 0 and seen[1] > 0 and seen[2] > 0, seen
    p.close()


END_TO_END = [("atom_n1_8.data", 1.0, 3), ("atom_n3_216.data", 3.0, 2)]


@pytest.mark.parametrize("name,right,cycles", END_TO_END, ids=[m[0] for m in END_TO_END])
def test_adaptive_run_is_unchanged(golden_dir, name, right, cycles):
    """the golden configurations (10 vacuum cells, Kelly marking) with and without the key: the same iteration counts, the
    same printed residuals and norms, the same refinement marks"""
    S = pkg().step50
    runs = {}
    for key in (False, True):
        p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous",
                                 cycles=cycles, r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR",
                                 refinement_estimator="Kelly", system_matrix_on_device=key))
        p.read_lammps(os.path.join(golden_dir, name))
        out = []
        for cycle in range(cycles):
            rep = p.run_cycle(cycle, on_device=True)
            assert p.system_matrix_on_device() == key
            out.append((rep, p.refine_flags(), p.matrix_shape("system")[1] if not key else p.device_system_matrix().nnz))
            if key:  # the printed Frobenius norm came from the device: against the exact sum over the host's values
                assert frobenius_close(rep["matrix_frobenius"], p.matrix("system").val), cycle
        runs[key] = out
        p.close()
    for cycle, ((r0, f0, nnz0), (r1, f1, nnz1)) in enumerate(zip(runs[False], runs[True])):
        for k in ("cg_iterations", "coarse_iterations", "starting_value", "convergence_value", "matrix_l1", "matrix_linf", "dofs", "active_cells",
                  "rhs_l2", "sol_l1", "sol_l2", "sol_linf"):
            assert r0[k] == r1[k], (cycle, k, r0[k], r1[k])
        assert nnz0 == nnz1
        assert np.array_equal(f0, f1), cycle


def test_2d_mesh_through_the_abi(ctx):
    inp = smr.quadrant_mesh_2d()
    assemble(ctx, inp)
    dev = ctx.get_system_matrix()
    assert smr.same_bits(dev, smr.assemble(inp)) and smr.same_bits(dev, smr.assemble_loops(inp))
    assert dev.nnz > 0 and np.any(dev.val == 0.0)  # the constrained rows keep their couplings as stored zeros


def test_invalid_arguments_are_refused_and_the_context_survives(ctx):
    good = smr.quadrant_mesh_2d()
    assemble(ctx, good)
    before = ctx.get_system_matrix()

    def changed(**kw):
        d = dict(vars(good))
        d.update(kw)
        return SimpleNamespace(**d)

    def with_entry(a, i, v):
        a = np.array(a)
        a.reshape(-1)[i] = v
        return a

    lp_dec = with_entry(good.line_ptr, len(good.line_ptr) - 2, good.line_ptr[-1] + 1)
    bad = {
        "dim": changed(dim=4),
        "dof below": changed(cell_dofs=with_entry(good.cell_dofs, 5, -1)),
        "dof above": changed(cell_dofs=with_entry(good.cell_dofs, 5, good.n_dofs)),
        "master": changed(line_master=with_entry(good.line_master, 0, good.n_dofs)),
        "line index": changed(constraint_of_dof=with_entry(good.constraint_of_dof, 0, len(good.line_ptr) - 1)),
        "line_ptr start": changed(line_ptr=with_entry(good.line_ptr, 0, -1)),
        "line_ptr decreases": changed(line_ptr=lp_dec),
        "level": changed(cell_level=with_entry(good.cell_level, 0, 16)),
        "null": changed(constraint_of_dof=np.zeros(0, dtype=np.int32)),
    }
    for what, inp in bad.items():
        with pytest.raises(capi().GMGError) as e:
            assemble(ctx, inp, validate=False)
        assert e.value.code == capi().ERR_INVALID and "gmg_assemble_system_matrix" in str(e.value), what
        assert smr.same_bits(ctx.get_system_matrix(), before), what  # nothing was touched
    assemble(ctx, good)
    assert smr.same_bits(ctx.get_system_matrix(), before)


def test_unsupported_on_a_communicator():
    c = capi().Context(1)
    c.comm_init(0, 1, capi().Context.unique_id())
    with pytest.raises(capi().GMGError) as e:
        assemble(c, smr.quadrant_mesh_2d())
    assert e.value.code == capi().ERR_UNSUPPORTED
    c.close()


def test_reset_then_another_mesh(ctx, golden_dir):
    assemble(ctx, smr.quadrant_mesh_2d())
    p = problem(golden_dir, "atom_n1_8.data", 1.0, 1)
    p.run_cycle(0, on_device=False)
    inp = p.system_assembly_inputs()
    assert ctx.L.gmg_reset(ctx.h, C.c_int(1)) == capi().OK
    with pytest.raises(capi().GMGError):
        ctx.get_system_matrix()
    assemble(ctx, inp)
    assert smr.same_bits(ctx.get_system_matrix(), p.matrix("system"))
    p.close()


def test_zero_cells(ctx):
    empty = SimpleNamespace(dim=3, n_dofs=5, cell_dofs=np.zeros((0, 8), dtype=np.int32), cell_level=np.zeros(0, dtype=np.uint8),
                            K_of_level=np.zeros((16, 8, 8)), constraint_of_dof=-np.ones(5, dtype=np.int32), line_ptr=None, line_master=None,
                            line_weight=None)
    assemble(ctx, empty)
    m = ctx.get_system_matrix()
    assert m.n_rows == 5 and m.nnz == 0 and np.array_equal(m.rowptr, np.zeros(6, dtype=np.int64))
    assert ctx.system_matrix_norms() == (0.0, 0.0, 0.0)
