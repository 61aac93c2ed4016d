"""gmg_output_patches and gmg_output_patches_resident on the MI355X (csrc/gmg_output.hpp) through the C
ABI, bit for bit against the restatement of tests/output_reference.py: point, solution, grad_phi and two gathered fields on
the meshes of tests/mesh_tables_cases.py and on hand-built forests -- one cell in a wavefront, the smallest meshes with
hanging nodes, cell counts that are no multiple of the 8 (3D) or 16 (2D) cells of a wavefront -- for several launch sizes and
launch shapes; the refusals; and whole runs of the driver whose files must equal those of a host-only run byte for byte."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import mesh_tables_cases as mtc
import mesh_tables_reference as mtr
import output_reference as ore
from gpu_util import capi, pkg
from test_system_matrix_cpu import problem as golden8_problem

pytestmark = pytest.mark.gpu

MESHES = ("A3", "G8-c2", "S2-c2", "S3-c1")
HAND = ("single-2d", "single-3d", "quadrant-2d", "edge-only-3d", "empty-2d", "empty-3d")
ORIGIN, H0 = -0.7, 0.3   # not dyadic: the product and the sum of a coordinate both round


@functools.lru_cache(maxsize=None)
def mesh(name):
    """namespace(dim, fc, cell_dofs [n_cells, nv], cell_level, keys, n_dofs, u, fields, ref): computed once, left unchanged"""
    if name in MESHES:
        x = mtc.case(name)
        fc, dim = x.fc, x.fc.dim
        cd, lv = np.asarray(x.sys.cell_dofs, dtype=np.int32).reshape(-1, 1 << dim), np.asarray(x.sys.cell_level, dtype=np.uint8)
        keys = np.asarray(x.ref.vertex_of_dof, dtype=np.uint64)
    else:
        fc = mtc.HAND_BUILT[name]()
        t, dim = mtr.build(fc), fc.dim
        cd, lv = np.asarray(t.cell_dofs, dtype=np.int32).reshape(-1, 1 << dim), np.asarray(t.cell_level, dtype=np.uint8)
        keys = np.asarray(t.vertex_of_dof, dtype=np.uint64)
    n = len(keys)
    rng = np.random.default_rng(len(name) * 1000 + n)
    u, f0, f1 = rng.normal(size=n), rng.normal(size=n), rng.uniform(-1e3, 1e3, size=n)
    cd, lv, keys = np.array(cd), np.array(lv), np.array(keys)   # (copies: the shared cases stay as they are)
    if len(cd):
        u[cd[-1, 2]] = -0.0             # a negative zero in the solution ...
        u[cd[-1, 0]] = 0.0              # ... above its neighbour +0.0 in y: g = (-0.0 - 0.0) / h = -0.0, grad_phi = +0.0
        u[cd[0, 1]] = u[cd[0, 0]]       # equal neighbours in x: g = +0.0, grad_phi = -0.0
        f0[cd[0, 0]] = -0.0
    ref = ore.patches(dim, cd, lv, keys, ORIGIN, H0, u, (f0, f1))
    if len(cd):
        assert np.signbit(ref.grad_phi[1, 0]) and ref.grad_phi[1, 0] == 0.0 and (np.signbit(ref.solution) & (ref.solution == 0.0)).any()
    for a in (cd, lv, keys, u, f0, f1):
        a.setflags(write=False)
    return SimpleNamespace(dim=dim, fc=fc, cell_dofs=cd, cell_level=lv, keys=keys, n_dofs=n, u=u, fields=(f0, f1), ref=ref)


def same(got, ref, what):
    assert ore.same_bits(got.point, ref.point), (what, "point")
    assert ore.same_bits(got.solution, ref.solution), (what, "solution")
    assert ore.same_bits(got.grad_phi, ref.grad_phi), (what, "grad_phi")
    assert len(got.patch_field) == len(ref.fields)
    for j, (g, r) in enumerate(zip(got.patch_field, ref.fields)):
        assert ore.same_bits(g, r), (what, "field", j)


def host_form(c, m, u=None, **kw):
    a = dict(dim=m.dim, cell_dofs=m.cell_dofs, cell_level=m.cell_level, vertex_of_dof=m.keys, origin=ORIGIN, h0=H0, u=u, fields=m.fields)
    a.update(kw)
    return c.output_patches(**a)


def build_tables(c, fc):
    c.build_mesh_tables(dim=fc.dim, n0=fc.n0, n_levels=fc.n_levels, level_ptr=fc.level_ptr, cell_coord=fc.cell_coord, cell_first_child=fc.cell_first_child,
                        level0_lexicographic=fc.level0_lexicographic)


@pytest.fixture()
def ctx():
    c = capi().Context(1)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ 1. both entries against the restatement

@pytest.mark.parametrize("name", MESHES + HAND)
def test_both_entries_equal_the_restatement(ctx, name):
    m = mesh(name)
    u = ctx.vector(m.n_dofs, m.u) if m.n_dofs else None
    # launches of 2^20 cells (one), of one cell and of 8 cells; by size, and one workgroup whose loop takes every turn
    for chunk, max_blocks in ((20, 0), (0, 0), (3, 0), (20, 1), (3, 1)):
        ctx.set_option("output_chunk_log2", chunk)
        ctx.set_option("assemble_max_blocks", max_blocks)
        got = host_form(ctx, m, u)
        same(got, m.ref, (name, chunk, max_blocks))
        assert got.build_ms >= 0.0
    # the resident form on the tables of the same forest: the tables number cells and DoFs as the restatement does
    build_tables(ctx, m.fc)
    t = ctx.get_mesh_tables()
    assert np.array_equal(np.asarray(t.cell_dofs).reshape(m.cell_dofs.shape), m.cell_dofs) and np.array_equal(t.vertex_of_dof, m.keys)
    for chunk, max_blocks in ((20, 0), (0, 0), (3, 1)):
        ctx.set_option("output_chunk_log2", chunk)
        ctx.set_option("assemble_max_blocks", max_blocks)
        same(ctx.output_patches_resident(ORIGIN, H0, u, fields=m.fields, n_u=m.n_dofs, dim=m.dim), m.ref, (name, "resident", chunk, max_blocks))
    if u is not None:
        u.free()


def test_null_outputs_are_skipped(ctx):
    m = mesh("edge-only-3d")
    u = ctx.vector(m.n_dofs, m.u)
    ctx.set_option("output_chunk_log2", 2)
    for want in (("point",), ("solution",), ("grad_phi",), ("patch_field",), ("point", "grad_phi"), ()):
        got = host_form(ctx, m, u, want=want)
        for k in ("point", "solution", "grad_phi"):
            assert ore.same_bits(getattr(got, k), getattr(m.ref, k) if k in want else np.zeros_like(getattr(m.ref, k))), (want, k)
        for g, r in zip(got.patch_field, m.ref.fields):
            assert ore.same_bits(g, r if "patch_field" in want else np.zeros_like(r)), want
    # no fields at all, and a field list with a NULL output next to a wanted one
    same(host_form(ctx, m, u, fields=None), SimpleNamespace(point=m.ref.point, solution=m.ref.solution, grad_phi=m.ref.grad_phi, fields=[]), "no fields")
    u.free()


# ------------------------------------------------------------------------------------------------ 2. the refusals

def refused(code, call, text=None):
    with pytest.raises(capi().GMGError) as e:
        call()
    assert e.value.code == code and "gmg_output_patches" in str(e.value) and (text is None or text in str(e.value)), str(e.value)
    return True


def test_refusals_found_on_the_host(ctx):
    A = capi()
    m = mesh("quadrant-2d")
    u = ctx.vector(m.n_dofs, m.u)
    bad_dof_hi, bad_dof_lo, bad_level = m.cell_dofs.copy(), m.cell_dofs.copy(), m.cell_level.copy()
    bad_dof_hi[3, 2], bad_dof_lo[0, 0], bad_level[-1] = m.n_dofs, -1, 14
    assert refused(A.ERR_INVALID, lambda: host_form(ctx, m, u, dim=4), "dim")
    assert refused(A.ERR_INVALID, lambda: host_form(ctx, m, u, dim=1), "dim")
    assert refused(A.ERR_INVALID, lambda: host_form(ctx, m, u, cell_level=bad_level), "level above 13")
    assert refused(A.ERR_INVALID, lambda: host_form(ctx, m, u, cell_dofs=bad_dof_hi), "DoF outside")
    assert refused(A.ERR_INVALID, lambda: host_form(ctx, m, u, cell_dofs=bad_dof_lo), "DoF outside")
    assert refused(A.ERR_INVALID, lambda: host_form(ctx, m, u, n_u=m.n_dofs + 1), "n_u")
    assert refused(A.ERR_INVALID, lambda: host_form(ctx, m, u, n_u=m.n_dofs - 1), "n_u")
    assert refused(A.ERR_INVALID, lambda: host_form(ctx, m, u, fields=[m.fields[0]] * 9), "n_fields")
    assert refused(A.ERR_INVALID, lambda: host_form(ctx, m, u, h0=0.0), "h0")
    assert refused(A.ERR_INVALID, lambda: host_form(ctx, m, u, h0=-1.0), "h0")
    assert refused(A.ERR_INVALID, lambda: host_form(ctx, m, None, n_u=m.n_dofs), "NULL")
    assert refused(A.ERR_INVALID, lambda: host_form(ctx, m, u, fields=[m.fields[0], None]), "NULL")
    for k in ("cell_dofs", "cell_level", "vertex_of_dof"):
        # (the view derives n_cells and n_dofs from the arrays it is given: say them)
        with pytest.raises(A.GMGError) as e:
            null_array(ctx, m, u, k)
        assert e.value.code == A.ERR_INVALID and "NULL" in str(e.value), (k, str(e.value))
    # a level of 13 is the last one taken, and a level-13 cell's edge is h0 / 8192
    lv13 = m.cell_level.copy()
    lv13[0] = 13
    got = host_form(ctx, m, u, cell_level=lv13)
    assert ore.same_bits(got.grad_phi, ore.patches(2, m.cell_dofs, lv13, m.keys, ORIGIN, H0, m.u).grad_phi)
    # the resident form: no tables; then tables, and the sibling's refusals of the remaining arguments
    assert refused(A.ERR_INVALID, lambda: ctx.output_patches_resident(ORIGIN, H0, u, dim=2), "no mesh tables")
    build_tables(ctx, m.fc)
    assert refused(A.ERR_INVALID, lambda: ctx.output_patches_resident(ORIGIN, H0, u, n_u=m.n_dofs + 1, dim=2), "n_u")
    assert refused(A.ERR_INVALID, lambda: ctx.output_patches_resident(ORIGIN, 0.0, u, dim=2), "h0")
    assert refused(A.ERR_INVALID, lambda: ctx.output_patches_resident(ORIGIN, H0, u, fields=[m.fields[0]] * 9, dim=2), "n_fields")
    assert refused(A.ERR_INVALID, lambda: ctx.output_patches_resident(ORIGIN, H0, None, n_u=m.n_dofs, dim=2), "NULL")
    same(ctx.output_patches_resident(ORIGIN, H0, u, fields=m.fields, dim=2), m.ref, "after the refusals")
    for key, value in (("output_chunk_log2", -1), ("output_chunk_log2", 31), ("output_chunk_log2", 2.5)):
        with pytest.raises(A.GMGError) as e:
            ctx.set_option(key, value)
        assert e.value.code == A.ERR_INVALID
    u.free()


def null_array(c, m, u, which):
    """gmg_output_patches with one mesh array NULL and the sizes of the whole mesh"""
    import ctypes as C

    A = capi()
    P = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))
    cd, lv, vk = (None if which == k else np.ascontiguousarray(a) for k, a in (("cell_dofs", m.cell_dofs), ("cell_level", m.cell_level), ("vertex_of_dof", m.keys)))
    c._chk(c.L.gmg_output_patches(c.h, C.c_int(m.dim), C.c_int64(len(m.cell_level)), P(cd, C.c_int32), P(lv, C.c_uint8), P(vk, C.c_uint64), C.c_int64(m.n_dofs),
                                  C.c_double(ORIGIN), C.c_double(H0), u.ptr, C.c_int64(m.n_dofs), C.c_int(0), None, None, None, None, None, None))


def test_unsupported_on_a_communicator():
    A = capi()
    c = A.Context(1)
    c.comm_init(0, 1, A.Context.unique_id())
    m = mesh("single-3d")
    u = c.vector(m.n_dofs, m.u)
    assert refused(A.ERR_UNSUPPORTED, lambda: host_form(c, m, u), "not on a communicator")
    assert refused(A.ERR_UNSUPPORTED, lambda: c.output_patches_resident(ORIGIN, H0, u, dim=3), "not on a communicator")
    u.free()
    c.close()


# ------------------------------------------------------------------------------------------------ 3. whole runs of the driver

RESIDENT_KEYS = dict(mesh_tables_on_device=True, system_matrix_on_device=True, level_matrices_on_device=True, rhs_from_cell_tables=True,
                     operators_from_resident_tables=True, estimator_on_device=True, refinement_on_device=True, transfer_on_device=True,
                     densities_from_resident_tables=True, estimator_from_resident_tables=True, energy_forces_from_resident_tables=True)


def test_driver_files_equal_those_of_a_host_only_run(tmp_path):
    """G8, cycles 0-2 on the device with every "... from resident tables" key set, against host-only cycles given the same
    solutions: the three files of every cycle byte for byte"""
    dev = golden8_problem(mtc.GOLDEN, "atom_n1_8.data", 1.0, 3, output_results=True, output_directory=str(tmp_path / "device"), **RESIDENT_KEYS)
    host = golden8_problem(mtc.GOLDEN, "atom_n1_8.data", 1.0, 3, output_results=True, output_directory=str(tmp_path / "host"))
    for cycle in range(3):
        dev.run_cycle(cycle, on_device=True)
        assert dev.operators_resident() and dev.output_path() == 2, (cycle, dev.log())
        x = dev.vector("solution")
        host.run_cycle(cycle, on_device=False)
        host.finish_cycle_with(x)
        assert host.output_path() == 0 and np.array_equal(host.vector("solution").view(np.uint64), x.view(np.uint64)), cycle
        a, b = ore.read_bytes(tmp_path / "device", cycle), ore.read_bytes(tmp_path / "host", cycle)
        assert a == b, (cycle, [len(v) for v in a], [len(v) for v in b])
        on, off = dev.output_patches(on_device=True), dev.output_patches(on_device=False)
        for g, h in zip(on, off):
            assert ore.same_bits(g, h), cycle
        f = ore.read_vtu(os.path.join(tmp_path / "device", ore.names(cycle)[0]))
        assert ore.same_bits(f.points, on[0]) and ore.same_bits(f.point_data["solution"], on[1]) and ore.same_bits(f.point_data["grad_phi"], on[2])
    assert len(np.unique(dev.system_assembly_inputs().cell_level)) > 1
    assert "Output results" not in dev.log(), dev.log()   # no fallback line
    dev.close()
    host.close()


def test_driver_falls_back_to_host_arrays_and_says_so_once(tmp_path):
    """the cycle runs on the device but the tables are not resident: gmg_output_patches on host arrays, the same bytes"""
    dev = golden8_problem(mtc.GOLDEN, "atom_n1_8.data", 1.0, 2, output_results=True, output_directory=str(tmp_path / "device"))
    host = golden8_problem(mtc.GOLDEN, "atom_n1_8.data", 1.0, 2, output_results=True, output_directory=str(tmp_path / "host"))
    for cycle in range(2):
        dev.run_cycle(cycle, on_device=True)
        assert dev.output_path() == 1
        host.run_cycle(cycle, on_device=False)
        host.finish_cycle_with(dev.vector("solution"))
        assert ore.read_bytes(tmp_path / "device", cycle) == ore.read_bytes(tmp_path / "host", cycle), cycle
    said = [l for l in dev.log().splitlines() if "Output results" in l]
    assert said == ["   Output results: patches from host arrays (Operators from resident tables did not take effect)"]
    dev.close()
    host.close()
