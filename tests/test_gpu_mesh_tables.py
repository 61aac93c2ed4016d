"""gmg_build_mesh_tables on the MI355X (csrc/gmg_mesh_tables.hpp) through the C ABI: DoF numbering,
constraint lines and level flags (src/step-50.cc:661-706: dof_handler.distribute_dofs / distribute_mg_dofs,
make_hanging_node_constraints, interpolate_boundary_values, MGConstrainedDoFs) against the restatement of
tests/mesh_tables_reference.py and the host driver's arrays on the meshes of tests/mesh_tables_cases.py and on hand-built
forests; the refusals; and whole runs of the driver with "Mesh tables on device" off and on.  Integer work with an exact
definition: every comparison is of equality."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import mesh_tables_cases as mtc
import mesh_tables_reference as mtr
from gpu_util import capi, pkg
from test_coef_matrix_cpu import step16_problem

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    c = capi().Context(1)
    yield c
    c.close()


def build(c, fc, **kw):
    a = dict(dim=fc.dim, n0=fc.n0, n_levels=fc.n_levels, level_ptr=fc.level_ptr, cell_coord=fc.cell_coord, cell_first_child=fc.cell_first_child,
             level0_lexicographic=fc.level0_lexicographic)
    a.update(kw)
    return c.build_mesh_tables(**a)


def tables(c, fc):
    """(active tables, [level tables]) of a build"""
    build(c, fc)
    return c.get_mesh_tables(), [c.get_mesh_level_tables(l) for l in range(fc.n_levels)]


def same(a, b):
    """two downloads of the tables hold the same arrays"""
    for x, y in zip([a[0]] + a[1], [b[0]] + b[1]):
        for k, v in vars(x).items():
            assert np.array_equal(v, getattr(y, k)), k
    return True


def refuses(c, code, fc, text=None, **kw):
    A = capi()
    with pytest.raises(A.GMGError) as e:
        build(c, fc, **kw)
    assert e.value.code == code and "gmg_build_mesh_tables" in str(e.value) and (text is None or text in str(e.value)), str(e.value)
    for get in (c.get_mesh_tables, lambda: c.get_mesh_level_tables(0)):   # the context holds no mesh tables
        with pytest.raises(A.GMGError) as e:
            get()
        assert e.value.code == A.ERR_INVALID


# ------------------------------------------------------------------------------------------------ 1. the meshes of the CPU tests

@pytest.mark.parametrize("name", sorted(mtc.CASES))
def test_device_equals_reference_and_host(name):
    x = mtc.case(name)
    first = None
    for max_blocks in (0, 1, 3):   # by size; one workgroup; three (every grid-stride loop iterates)
        c = capi().Context(1)
        c.set_option("assemble_max_blocks", max_blocks)
        got = tables(c, x.fc)
        c.close()
        mtc.same_tables(got[0], x.ref, (name, max_blocks))
        for l, (g, r) in enumerate(zip(got[1], x.ref.levels)):
            mtc.same_level(g, r, (name, max_blocks, l))
        first = first or got
        assert same(first, got)
    # and the host's arrays themselves (the lines are the host's before close: tests/test_mesh_tables_cpu.py)
    t, lv = first
    assert np.array_equal(t.cell_dofs.reshape(x.sys.cell_dofs.shape), x.sys.cell_dofs) and np.array_equal(t.cell_level, x.sys.cell_level)
    assert np.array_equal(t.constraint_of_dof, x.sys.constraint_of_dof) and t.n_lines == len(x.sys.line_inhomogeneity)
    for l, (g, h) in enumerate(zip(lv, x.levels)):
        assert np.array_equal(g.cell_dofs.reshape(h.cell_dofs.shape), h.cell_dofs) and np.array_equal(g.dof_flags, h.dof_flags), (name, l)


def test_two_builds_in_a_row(ctx):
    """the second build replaces the first: the same arrays, and those of another forest in between"""
    x, y = mtc.case("B3"), mtc.case("S2-c2")
    a = tables(ctx, x.fc)
    b = tables(ctx, x.fc)
    assert same(a, b)
    other = tables(ctx, y.fc)
    mtc.same_tables(other[0], y.ref)
    assert same(a, tables(ctx, x.fc))


# ------------------------------------------------------------------------------------------------ 2. hand-built forests

@pytest.mark.parametrize("name", sorted(mtc.HAND_BUILT))
def test_hand_built_forests(ctx, name):
    fc = mtc.HAND_BUILT[name]()
    ref = mtr.build(fc)
    for max_blocks in (0, 1):
        ctx.set_option("assemble_max_blocks", max_blocks)
        t, lv = tables(ctx, fc)
        mtc.same_tables(t, ref, name)
        assert len(lv) == len(ref.levels)
        for l, (g, r) in enumerate(zip(lv, ref.levels)):
            mtc.same_level(g, r, (name, l))


def test_zero_levels_and_null_arrays(ctx):
    """no cells at all: with one empty level, and with no level and NULL cell arrays"""
    t, lv = tables(ctx, mtr.empty(3))
    assert (t.n_cells, t.n_dofs, t.n_lines) == (0, 0, 0) and t.line_ptr.tolist() == [0] and lv[0].n_dofs == 0
    none = SimpleNamespace(dim=2, n0=(1, 1, 1), n_levels=0, level_ptr=[0], cell_coord=None, cell_first_child=None, level0_lexicographic=True)
    build(ctx, none)
    assert ctx.get_mesh_tables().n_dofs == 0
    with pytest.raises(capi().GMGError) as e:
        ctx.get_mesh_level_tables(0)
    assert e.value.code == capi().ERR_INVALID


# ------------------------------------------------------------------------------------------------ 3. the refusals

def changed(fc, **kw):
    d = dict(vars(fc))
    d.update(kw)
    return SimpleNamespace(**d)


def test_refusals_found_on_the_host(ctx):
    A = capi()
    good = mtr.quadrant_2d()
    coord = lambda i, d, v: [[v if (j, e) == (i, d) else x for e, x in enumerate(c)] for j, c in enumerate(good.cell_coord)]
    child = lambda i, v: [v if j == i else x for j, x in enumerate(good.cell_first_child)]
    bad = {
        "dim": changed(good, dim=4),
        "coord null": changed(good, cell_coord=None),
        "first_child null": changed(good, cell_first_child=None),
        "level_ptr null": changed(good, level_ptr=None),
        "n0 null": changed(good, n0=None),
        "level_ptr decreases": changed(good, level_ptr=[0, 5, 4]),
        "level_ptr starts above 0": changed(good, level_ptr=[1, 4, 8]),
        "14 levels": changed(good, level_ptr=[0, 4, 8] + [8] * 12, n_levels=14),
        "n0 = 0": changed(good, n0=(2, 0, 1)),
        "n0 = 512": changed(good, n0=(512, 2, 1)),
        "x outside": changed(good, cell_coord=coord(1, 0, 2)),
        "negative": changed(good, cell_coord=coord(2, 1, -1)),
        "z in 2D": changed(good, cell_coord=coord(0, 2, 1)),
        "fine outside": changed(good, cell_coord=coord(5, 0, 4)),
        "first_child beyond": changed(good, cell_first_child=child(0, 1)),
        "first_child on the last level": changed(good, cell_first_child=child(6, 0)),
        "not the full lattice": changed(good, n0=(3, 2, 1)),
        "not lexicographic": changed(good, cell_coord=[good.cell_coord[1], good.cell_coord[0]] + good.cell_coord[2:]),
    }
    for what, fc in bad.items():
        build(ctx, good)   # something to lose
        refuses(ctx, A.ERR_INVALID, fc)
    mtc.same_tables(tables(ctx, good)[0], mtr.build(good))   # the context survives
    # sizes beyond 32-bit slots are refused before any array is read
    huge = SimpleNamespace(dim=3, n0=(511, 511, 511), n_levels=1, level_ptr=[0, 1 << 28], cell_coord=[[0, 0, 0]], cell_first_child=[-1], level0_lexicographic=False)
    refuses(ctx, A.ERR_UNSUPPORTED, huge, "2^31 slots")


def test_refusals_found_on_the_device(ctx):
    A = capi()
    good = mtr.quadrant_2d(False)
    twice = changed(good, cell_coord=good.cell_coord[:5] + [good.cell_coord[4]] + good.cell_coord[6:])
    for max_blocks in (0, 1):
        ctx.set_option("assemble_max_blocks", max_blocks)
        refuses(ctx, A.ERR_INVALID, twice, "the same cell appears twice")
        refuses(ctx, A.ERR_INVALID, mtr.unbalanced_2d(), "not 2:1 balanced")
    with pytest.raises(mtr.Unbalanced):
        mtr.build(mtr.unbalanced_2d())
    mtc.same_tables(tables(ctx, good)[0], mtr.build(good))


def test_unsupported_on_a_communicator():
    A = capi()
    c = A.Context(1)
    c.comm_init(0, 1, A.Context.unique_id())
    refuses(c, A.ERR_UNSUPPORTED, mtr.quadrant_2d(), "not on a communicator")
    c.close()


def test_reset_drops_the_tables(ctx):
    A = capi()
    fc = mtr.edge_only_3d()
    build(ctx, fc)
    assert ctx.get_mesh_tables().n_hanging == 9
    assert ctx.L.gmg_reset(ctx.h, C.c_int(2)) == A.OK
    with pytest.raises(A.GMGError) as e:
        ctx.get_mesh_tables()
    assert e.value.code == A.ERR_INVALID
    assert tables(ctx, fc)[0].n_hanging == 9


def test_no_leak_over_six_rounds():
    """as tests/test_gpu_lifecycle.py: build, download, destroy, six times; the free device memory after the last round equals
    that after the first"""
    import torch

    x = mtc.case("B3")
    free = []
    for _ in range(6):
        c = capi().Context(1)
        tables(c, x.fc)
        tables(c, mtr.quadrant_2d())   # a build over a build
        c.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    print("free device memory after each round, relative to the first:", [f - free[0] for f in free])
    assert free[-1] == free[0], free


# ------------------------------------------------------------------------------------------------ 4. whole runs of the driver

SKIP_KEYS = ("solve_seconds", "build_matrices_ms")   # times
# energy_norm_error is an OpenMP reduction over the cells in the order the threads finish (postprocess_error_in_energy_norm): its
# last bits differ between two runs of one configuration.  A sum of n non-negative terms in any order, then a square root: two
# such values differ by at most (n + 2) 2^-53 relative, each from the exact one.
UNORDERED_SUMS = ("energy_norm_error",)
OTHER_KEYS_ON = dict(system_matrix_on_device=True, level_matrices_on_device=True, rhs_from_cell_tables=True, estimator_on_device=True,
                     analytical_on_device=True)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def norm_lines(log):
    """the driver's log -- counts, norms, residuals, energies; it prints no times -- without the one unordered sum"""
    return [l for l in log.splitlines() if "energy norm" not in l]


def driver_runs(make, cycles):
    """the same run with the key off and on: per cycle the report, the marks, the right-hand side and the solution, and the log.
    Everything but the times must be equal."""
    runs = {}
    for key in (False, True):
        p = make(key)
        out = []
        for cycle in range(cycles):
            rep = p.run_cycle(cycle, on_device=True)
            assert p.mesh_tables_on_device() == key, cycle
            out.append((rep, p.refine_flags(), p.vector("rhs"), p.vector("solution"), p.system_assembly_inputs(),
                        [p.level_assembly_inputs(l) for l in range(p.n_levels())], p.dof_coordinates()))
        assert "Mesh tables on device" not in p.log(), p.log()   # no fallback line
        runs[key] = (out, norm_lines(p.log()))
        p.close()
    assert runs[False][1] == runs[True][1]
    for cycle, (a, b) in enumerate(zip(runs[False][0], runs[True][0])):
        for k in a[0]:
            if k in UNORDERED_SUMS:
                assert abs(a[0][k] - b[0][k]) <= 2 * (a[0]["active_cells"] + 2) * 2.0 ** -53 * abs(a[0][k]), (cycle, k, a[0][k], b[0][k])
            elif k not in SKIP_KEYS:
                assert repr(a[0][k]) == repr(b[0][k]), (cycle, k, a[0][k], b[0][k])
        assert np.array_equal(a[1], b[1]), cycle
        assert np.array_equal(bits(a[2]), bits(b[2])) and np.array_equal(bits(a[3]), bits(b[3])), cycle
        # the tables the other device entries take, as the driver holds them after either path (the lines closed)
        for k in ("cell_dofs", "cell_level", "constraint_of_dof", "line_ptr", "line_master"):
            assert np.array_equal(getattr(a[4], k), getattr(b[4], k)), (cycle, k)
        assert np.array_equal(bits(a[4].line_weight), bits(b[4].line_weight)) and np.array_equal(bits(a[4].line_inhomogeneity), bits(b[4].line_inhomogeneity))
        for l, (u, v) in enumerate(zip(a[5], b[5])):
            assert np.array_equal(u.cell_dofs, v.cell_dofs) and np.array_equal(u.dof_flags, v.dof_flags), (cycle, l)
        assert np.array_equal(bits(a[6]), bits(b[6])), cycle
    return runs


def golden_make(golden_dir, name, right, cycles, smoother, **more):
    S = pkg().step50

    def make(key):
        p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=cycles,
                                 r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother=smoother,
                                 refinement_estimator="Kelly", mesh_tables_on_device=key, **more))
        p.read_lammps(os.path.join(golden_dir, name))
        return p

    return make


GOLDEN_RUNS = [("atom_n1_8.data", 1.0, 3, "SSOR", {}), ("atom_n1_8.data", 1.0, 3, "SSOR", OTHER_KEYS_ON), ("atom_n3_216.data", 3.0, 2, "SSOR", {})]


@pytest.mark.parametrize("name,right,cycles,smoother,more", GOLDEN_RUNS, ids=[f"{m[0]}-{m[3]}{'-all' if m[4] else ''}" for m in GOLDEN_RUNS])
def test_adaptive_run_is_unchanged(golden_dir, name, right, cycles, smoother, more):
    """the golden configurations (10 vacuum cells, Kelly marking): equal iteration counts, printed norms, residuals, thresholds,
    energies, marks, and the bits of system_rhs and of the distributed solution"""
    runs = driver_runs(golden_make(golden_dir, name, right, cycles, smoother, **more), cycles)
    last = runs[True][0][-1][0]
    assert len(last["dofs_by_level"]) >= 2 and last["cg_iterations"] >= 1


@pytest.mark.parametrize("dim,refine", ((2, 3), (3, 2)))
def test_step16_run_is_unchanged(dim, refine):
    runs = driver_runs(lambda key: step16_problem(dim, refine, 3, mesh_tables_on_device=key), 3)
    assert len(runs[True][0][-1][0]["dofs_by_level"]) >= refine + 2


def test_cellwise_level0_run_is_unchanged(golden_dir):
    runs = driver_runs(golden_make(golden_dir, "atom_n1_8.data", 1.0, 2, "SSOR", level0_numbering="cell-wise"), 2)
    assert runs[True][0][-1][0]["cg_iterations"] >= 1


def test_host_cycle_keeps_the_host_loops(golden_dir):
    """a cycle that does not run on the device: one line says why, the tables are the host's"""
    p = golden_make(golden_dir, "atom_n1_8.data", 1.0, 1, "SSOR")(True)
    q = golden_make(golden_dir, "atom_n1_8.data", 1.0, 1, "SSOR")(False)
    p.run_cycle(0, on_device=False)
    q.run_cycle(0, on_device=False)
    assert not p.mesh_tables_on_device() and np.array_equal(bits(p.vector("rhs")), bits(q.vector("rhs")))
    assert p.log().count("Mesh tables on device: not applicable (the cycle does not run on the device)") == 1
    p.close()
    q.close()


def test_distributed_run_keeps_the_host_loops(golden_dir):
    """a run on a communicator (one rank): one line says why, the result is the host path's"""
    p = golden_make(golden_dir, "atom_n1_8.data", 1.0, 1, "SSOR")(True)
    q = golden_make(golden_dir, "atom_n1_8.data", 1.0, 1, "SSOR")(False)
    p.set_communicator(0, 1, capi().Context.unique_id())
    r1, r0 = p.run_cycle(0, on_device=True), q.run_cycle(0, on_device=True)
    assert not p.mesh_tables_on_device() and np.array_equal(bits(p.vector("rhs")), bits(q.vector("rhs")))
    assert np.array_equal(bits(p.vector("solution")), bits(q.vector("solution"))) and r1["cg_iterations"] == r0["cg_iterations"]
    assert p.log().count("Mesh tables on device: not applicable (the run is distributed)") == 1
    p.close()
    q.close()
