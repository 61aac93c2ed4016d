"""gmg_refine_forest, gmg_transfer_solution and gmg_build_face_table on the MI355X (csrc/gmg_refine.hpp)
through the C ABI: Forest::refine_flagged, the solution transfer of LaplaceProblem::refine_grid (src/step-50.cc:1095-1121) and
LaplaceProblem::face_table against the restatement of tests/refine_reference.py and the host driver's arrays on the steps of
tests/refine_cases.py; the refusals; and whole runs of the driver with "Refinement on device" off and on.  Integer work and
sums in a fixed order: every comparison is of equality, the transferred solution bit for bit."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import mesh_tables_reference as mtr
import refine_cases as rc
import refine_reference as rr
from gpu_util import capi, pkg
from test_coef_matrix_cpu import step16_problem
from test_gpu_mesh_tables import SKIP_KEYS, UNORDERED_SUMS, norm_lines

pytestmark = pytest.mark.gpu

bits = rc.bits


@pytest.fixture()
def ctx():
    c = capi().Context(1)
    yield c
    c.close()


def kw(fc, **more):
    a = dict(dim=fc.dim, n0=fc.n0, n_levels=fc.n_levels, level_ptr=fc.level_ptr, cell_coord=fc.cell_coord, cell_first_child=fc.cell_first_child)
    a.update(more)
    return a


def refine(c, fc, flag):
    r = c.refine_forest(flag=flag, **kw(fc))
    g = c.get_refined_forest()
    assert (r.n_levels, r.n_cells, r.n_split) == (g.n_levels, g.n_cells, g.n_split) and g.n_cells == len(g.cell_first_child)
    return g


def transfer(c, new_fc, old_vertex, u_old, new_vertex, cons, fill=None):
    """u_new of gmg_transfer_solution (None for an empty mesh: the vectors are then NULL); fill: what u_new holds before"""
    A = capi()
    uo = A.DeviceVector(c, len(old_vertex)).upload(u_old) if len(old_vertex) else None
    un = A.DeviceVector(c, len(new_vertex)) if len(new_vertex) else None
    if un is not None and fill is not None:
        un.upload(np.full(len(new_vertex), fill))
    try:
        c.transfer_solution(old_vertex_of_dof=old_vertex, u_old=uo, new_vertex_of_dof=new_vertex, constraint_of_dof=cons, u_new=un, **kw(new_fc))
        return un.download() if un is not None else np.zeros(0)
    except A.GMGError as e:
        e.u_new = un.download() if un is not None else None
        raise
    finally:
        for v in (uo, un):
            if v is not None:
                v.free()


def same_refined(got, ref, what=""):
    rc.same_forest(got, ref.forest, what)
    assert np.array_equal(got.cell_parent, np.asarray(ref.cell_parent, dtype=np.int32)), (what, "cell_parent")
    assert np.array_equal(got.closed_flag, np.asarray(ref.closed_flag, dtype=np.uint8)), (what, "closed_flag")
    assert got.n_split == ref.n_split, (what, got.n_split, ref.n_split)


def all_three(c, s):
    """(refined forest, u_new, face table of the new forest) of one step"""
    g = refine(c, s.fc, s.flag)
    new = SimpleNamespace(dim=s.fc.dim, n0=s.fc.n0, n_levels=g.n_levels, level_ptr=g.level_ptr, cell_coord=g.cell_coord, cell_first_child=g.cell_first_child)
    return g, transfer(c, new, s.old_vertex, s.u_old, s.new_vertex, s.cons), c.build_face_table(**kw(new))


def same_outputs(a, b):
    for k, v in vars(a[0]).items():
        assert np.array_equal(v, getattr(b[0], k)), k
    assert np.array_equal(bits(a[1]), bits(b[1]))
    assert np.array_equal(a[2].face_kind, b[2].face_kind) and np.array_equal(a[2].face_cell, b[2].face_cell)
    return True


# ------------------------------------------------------------------------------------------------ 1. the steps of the CPU tests

@pytest.mark.parametrize("name", rc.STEPS)
def test_device_equals_reference_and_host(name):
    s = rc.step(name)
    first = None
    for max_blocks in (0, 1, 3):   # by size; one workgroup; three (every grid-stride loop iterates)
        c = capi().Context(1)
        c.set_option("assemble_max_blocks", max_blocks)
        got = all_three(c, s)
        old_faces = c.build_face_table(**kw(s.fc))
        c.close()
        same_refined(got[0], s.ref, (name, max_blocks))
        assert np.array_equal(bits(got[1]), bits(s.ref_u)), (name, max_blocks)
        first = first or got
        assert same_outputs(first, got)
        # and the host's arrays themselves
        rc.same_forest(got[0], s.new_fc, name)
        assert np.array_equal(got[0].cell_parent, s.parent) and np.array_equal(got[0].closed_flag, s.closed)
        assert np.array_equal(bits(got[1]), bits(s.u_new)), (name, max_blocks)
        assert np.array_equal(got[2].face_kind, s.new_faces[0]) and np.array_equal(got[2].face_cell, s.new_faces[1]), (name, max_blocks)
        assert np.array_equal(old_faces.face_kind, s.faces[0]) and np.array_equal(old_faces.face_cell, s.faces[1]), (name, max_blocks)
    k, cell = rr.face_table(s.new_fc)
    assert np.array_equal(first[2].face_kind, k) and np.array_equal(first[2].face_cell, cell)


@pytest.mark.parametrize("name", sorted(rc.HAND_BUILT))
def test_hand_built_steps(ctx, name):
    s = rc.hand(name)
    k, cell = rr.face_table(s.ref.forest)
    for max_blocks in (0, 1):
        ctx.set_option("assemble_max_blocks", max_blocks)
        g, u, faces = all_three(ctx, s)
        same_refined(g, s.ref, (name, max_blocks))
        assert np.array_equal(bits(u), bits(s.ref_u)), (name, max_blocks)
        assert faces.n_active == len(k) and np.array_equal(faces.face_kind, k) and np.array_equal(faces.face_cell, cell), (name, max_blocks)
        # without constraint_of_dof nothing is zeroed
        free = transfer(ctx, s.ref.forest, s.old_vertex, s.u_old, s.new_vertex, None)
        assert np.array_equal(bits(free), bits(rr.transfer(s.ref.forest, s.old_vertex, s.u_old, s.new_vertex, None)))


def test_no_levels_and_null_arrays(ctx):
    none = SimpleNamespace(dim=2, n0=(1, 1, 1), n_levels=0, level_ptr=[0], cell_coord=None, cell_first_child=None)
    g = refine(ctx, none, None)
    assert (g.n_levels, g.n_cells, g.n_split) == (0, 0, 0) and g.level_ptr.tolist() == [0]
    assert len(transfer(ctx, none, [], [], [], None)) == 0
    assert ctx.build_face_table(**kw(none)).n_active == 0


def test_two_calls_in_a_row(ctx):
    """the second call replaces the first: the same arrays, and those of another step in between"""
    x, y = rc.step("G8:0->1"), rc.step("S2:1->2")
    a = all_three(ctx, x)
    assert same_outputs(a, all_three(ctx, x))
    same_refined(all_three(ctx, y)[0], y.ref)
    assert same_outputs(a, all_three(ctx, x))


# ------------------------------------------------------------------------------------------------ 2. the refusals

def changed(fc, **more):
    d = dict(vars(fc))
    d.update(more)
    return SimpleNamespace(**d)


def entries(c, s):
    """the three entries on one step's arrays, each as (name, call(forest, **overrides))"""
    def t(fc, **o):
        a = dict(old_vertex=s.old_vertex, u_old=s.u_old, new_vertex=s.new_vertex, cons=s.cons)
        a.update(o)
        return transfer(c, fc, a["old_vertex"], a["u_old"], a["new_vertex"], a["cons"], fill=7.0)
    return (("gmg_refine_forest", lambda fc, **o: c.refine_forest(flag=o.get("flag", [0] * len(fc.cell_first_child or [])), **kw(fc))),
            ("gmg_transfer_solution", t), ("gmg_build_face_table", lambda fc, **o: c.build_face_table(**kw(fc))))


def refuses(c, code, call, who, text=None):
    A = capi()
    before = c.get_refined_forest()
    with pytest.raises(A.GMGError) as e:
        call()
    assert e.value.code == code and who in str(e.value) and (text is None or text in str(e.value)), str(e.value)
    if getattr(e.value, "u_new", None) is not None:
        assert np.all(e.value.u_new == 7.0)          # u_new is not written
    after = c.get_refined_forest()                   # and the context is what it was
    for k, v in vars(before).items():
        assert np.array_equal(v, getattr(after, k)), k


def test_refusals_found_on_the_host(ctx):
    A = capi()
    s = rc.hand("lattice-2x2")
    good = s.ref.forest   # 2 x 2 with one cell refined
    s = SimpleNamespace(old_vertex=s.new_vertex, u_old=s.ref_u, new_vertex=s.new_vertex, cons=s.cons)
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
    }
    refine(ctx, good, [0] * 8)   # something to lose
    for who, call in entries(ctx, s):
        for what, fc in bad.items():
            refuses(ctx, A.ERR_INVALID, lambda: call(fc), who)
        huge = SimpleNamespace(dim=3, n0=(511, 511, 511), n_levels=1, level_ptr=[0, 1 << 28], cell_coord=[[0, 0, 0]], cell_first_child=[-1])
        refuses(ctx, A.ERR_UNSUPPORTED, lambda: call(huge, flag=[0]), who, "2^31 slots")
    # NULL arrays of nonzero length that belong to one entry
    name, call = entries(ctx, s)[0]
    refuses(ctx, A.ERR_INVALID, lambda: call(good, flag=None), name, "NULL")
    with pytest.raises(A.GMGError) as e:   # (vectors of n entries, vertex lists NULL)
        ctx.transfer_solution(old_vertex_of_dof=None, u_old=None, new_vertex_of_dof=None, constraint_of_dof=None, u_new=None, n_old=3, n_new=3, **kw(good))
    assert e.value.code == A.ERR_INVALID
    with pytest.raises(A.GMGError) as e:   # gmg_build_face_table: one of the two arrays NULL
        na = C.c_int64(0)
        args, keep = ctx._forest_args(good.dim, good.n0, good.level_ptr, good.cell_coord, good.cell_first_child, None)
        kind = np.full(7 * 4, 9, dtype=np.uint8)
        ctx._chk(ctx.L.gmg_build_face_table(ctx.h, *args, C.byref(na), kind.ctypes.data_as(C.POINTER(C.c_uint8)), None, None))
    assert e.value.code == A.ERR_INVALID and np.all(kind == 9)
    same_refined(refine(ctx, rc.hand("lattice-2x2").fc, rc.hand("lattice-2x2").flag), rc.hand("lattice-2x2").ref)   # the context survives


def twice_refined_2d():
    """a 2 x 1 lattice: cell 0 refined, its child at (1, 0) refined again -- cell 1 sees a child that is not active across its face"""
    return mtr.forest(2, (2, 1, 1), [[(0, 0, 0, 0), (1, 0, 0, -1)], [(0, 0, 0, -1), (1, 0, 0, 0), (0, 1, 0, -1), (1, 1, 0, -1)], mtr._children(1, 0, 0, 2)], True)


def test_refusals_found_on_the_device(ctx):
    A = capi()
    s = rc.hand("staircase-2d")
    new = s.ref.forest
    refine(ctx, s.fc, s.flag)
    twice = changed(s.fc, cell_coord=s.fc.cell_coord[:5] + [s.fc.cell_coord[4]] + s.fc.cell_coord[6:])
    hole, deep = rr.hole_2d(), rr.corner_12()
    for max_blocks in (0, 1):
        ctx.set_option("assemble_max_blocks", max_blocks)
        for who, call in entries(ctx, s)[::2]:   # (the two entries that look cells up)
            refuses(ctx, A.ERR_INVALID, lambda: call(twice), who, "appears twice")
        # gmg_refine_forest: not vertex-balanced; a split on level 12
        refuses(ctx, A.ERR_INVALID, lambda: ctx.refine_forest(flag=rr.flags_at(hole, [(1, 1, 0, 0)]), **kw(hole)), "gmg_refine_forest", "not vertex-balanced")
        refuses(ctx, A.ERR_UNSUPPORTED, lambda: ctx.refine_forest(flag=rr.flags_at(deep, [(12, 0, 0, 0)]), **kw(deep)), "gmg_refine_forest", "level 12")
        # gmg_transfer_solution: a parent vertex without an old value; the same vertex twice; a new vertex list that lacks one
        refuses(ctx, A.ERR_INVALID, lambda: transfer(ctx, new, s.old_vertex[1:], s.u_old[1:], s.new_vertex, s.cons, fill=7.0), "gmg_transfer_solution",
                "without a value")
        refuses(ctx, A.ERR_INVALID, lambda: transfer(ctx, new, s.old_vertex, s.u_old, s.new_vertex[:-1] + s.new_vertex[:1], s.cons[:], fill=7.0),
                "gmg_transfer_solution", "appears twice")
        i = next(i for i, k in enumerate(s.new_vertex) if k not in set(s.old_vertex))
        refuses(ctx, A.ERR_INVALID, lambda: transfer(ctx, new, s.old_vertex, s.u_old, s.new_vertex[:i] + s.new_vertex[i + 1:], s.cons[:i] + s.cons[i + 1:], fill=7.0),
                "gmg_transfer_solution", "without a value")
        # gmg_build_face_table: a kind-3 neighbour that is missing, a kind-2 child that is not active
        for fc in (hole, twice_refined_2d()):
            refuses(ctx, A.ERR_INVALID, lambda: ctx.build_face_table(**kw(fc)), "gmg_build_face_table", "mesh not 2:1 balanced across a face")
        with pytest.raises(rr.Unbalanced):
            rr.face_table(twice_refined_2d())
    with pytest.raises(rr.NoValue):
        rr.transfer(new, s.old_vertex[1:], s.u_old[1:], s.new_vertex, s.cons)
    assert rr.refine(deep, rr.flags_at(deep, [(11, 1, 1, 0)])).n_split >= 1
    same_refined(refine(ctx, deep, rr.flags_at(deep, [(11, 1, 1, 0)])), rr.refine(deep, rr.flags_at(deep, [(11, 1, 1, 0)])))   # level 11 may be split


def test_unsupported_on_a_communicator():
    A = capi()
    c = A.Context(1)
    s = rc.hand("lattice-2x2")
    refine(c, s.fc, s.flag)
    c.comm_init(0, 1, A.Context.unique_id())
    for who, call in entries(c, SimpleNamespace(old_vertex=s.old_vertex, u_old=s.u_old, new_vertex=s.old_vertex, cons=None)):
        refuses(c, A.ERR_UNSUPPORTED, lambda: call(s.fc), who, "not on a communicator")
    c.close()


def test_reset_drops_the_refined_forest(ctx):
    A = capi()
    s = rc.hand("edge-3d")
    assert refine(ctx, s.fc, s.flag).n_split == 4
    assert ctx.L.gmg_reset(ctx.h, C.c_int(2)) == A.OK
    with pytest.raises(A.GMGError) as e:
        ctx.get_refined_forest()
    assert e.value.code == A.ERR_INVALID
    assert refine(ctx, s.fc, s.flag).n_split == 4


def test_no_leak_over_six_rounds():
    """as tests/test_gpu_lifecycle.py: the three entries, a refinement over a refinement, destroy, six times; the free device
    memory after the last round equals that after the first"""
    import torch

    x, y = rc.step("B3:0->1"), rc.hand("staircase-2d")
    free = []
    for _ in range(6):
        c = capi().Context(1)
        all_three(c, x)
        all_three(c, y)
        c.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    print("free device memory after each round, relative to the first:", [f - free[0] for f in free])
    assert free[-1] == free[0], free


# ------------------------------------------------------------------------------------------------ 3. whole runs of the driver

OTHER_KEYS_ON = dict(system_matrix_on_device=True, level_matrices_on_device=True, rhs_from_cell_tables=True, estimator_on_device=True,
                     analytical_on_device=True, mesh_tables_on_device=True)


def driver_runs(make, cycles):
    """the same run with the key off and on: per cycle the report, the marks and their closure, the forest, the right-hand side,
    the initial guess and the solution, and the log.  Everything but the times must be equal."""
    runs = {}
    for key in (False, True):
        p = make(key)
        out = []
        for cycle in range(cycles):
            rep = p.run_cycle(cycle, on_device=True)
            assert p.refined_on_device() == (key and cycle > 0), cycle
            out.append((rep, p.refine_flags(), p.vector("rhs"), p.vector("solution"), p.vector("initial_guess"), p.forest_cells(), p.forest_parents(),
                        p.closed_flags(), p.estimator_inputs()))
        assert "Refinement on device" not in p.log(), p.log()   # no fallback line
        runs[key] = (out, norm_lines(p.log()))
        p.close()
    assert runs[False][1] == runs[True][1]
    for cycle, (a, b) in enumerate(zip(runs[False][0], runs[True][0])):
        for k in a[0]:
            if k in UNORDERED_SUMS:
                assert abs(a[0][k] - b[0][k]) <= 2 * (a[0]["active_cells"] + 2) * 2.0 ** -53 * abs(a[0][k]), (cycle, k, a[0][k], b[0][k])
            elif k not in SKIP_KEYS:
                assert repr(a[0][k]) == repr(b[0][k]), (cycle, k, a[0][k], b[0][k])
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[7], b[7]) and np.array_equal(a[6], b[6]), cycle
        for i in (2, 3, 4):
            assert np.array_equal(bits(a[i]), bits(b[i])), (cycle, i)
        for k in ("n_levels", "level_ptr", "cell_coord", "cell_first_child"):
            assert np.array_equal(getattr(a[5], k), getattr(b[5], k)), (cycle, k)
        assert np.array_equal(a[8].face_kind, b[8].face_kind) and np.array_equal(a[8].face_cell, b[8].face_cell), cycle
    return runs


def golden_make(golden_dir, name, right, cycles, smoother, **more):
    S = pkg().step50

    def make(key):
        p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=cycles,
                                 r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother=smoother,
                                 refinement_estimator="Kelly", refinement_on_device=key, **more))
        p.read_lammps(os.path.join(golden_dir, name))
        return p

    return make


GOLDEN_RUNS = [("atom_n1_8.data", 1.0, 3, "SSOR", {}), ("atom_n1_8.data", 1.0, 3, "SSOR", OTHER_KEYS_ON), ("atom_n3_216.data", 3.0, 2, "SSOR", {})]


@pytest.mark.parametrize("name,right,cycles,smoother,more", GOLDEN_RUNS, ids=[f"{m[0]}-{m[3]}{'-all' if m[4] else ''}" for m in GOLDEN_RUNS])
def test_adaptive_run_is_unchanged(golden_dir, name, right, cycles, smoother, more):
    """the golden configurations (10 vacuum cells, Kelly marking): equal iteration counts, printed norms, residuals, thresholds,
    energies, marks, forests, and the bits of system_rhs, of the initial guess and of the distributed solution"""
    runs = driver_runs(golden_make(golden_dir, name, right, cycles, smoother, **more), cycles)
    last = runs[True][0][-1][0]
    assert len(last["dofs_by_level"]) >= 2 and last["cg_iterations"] >= 1


@pytest.mark.parametrize("dim,refine_times", ((2, 3), (3, 2)))
def test_step16_run_is_unchanged(dim, refine_times):
    runs = driver_runs(lambda key: step16_problem(dim, refine_times, 3, refinement_on_device=key), 3)
    assert len(runs[True][0][-1][0]["dofs_by_level"]) >= refine_times + 2


def test_refine_with_flags_on_either_path(golden_dir):
    """Problem.refine_with_flags: the same marks through the host loops and through the device entries"""
    out = []
    for key in (False, True):
        p = golden_make(golden_dir, "atom_n1_8.data", 1.0, 2, "SSOR")(key)
        p.run_cycle(0, on_device=True)
        flags = p.refine_flags()
        flags[::7] = 1
        p.refine_with_flags(flags, on_device=True)
        assert p.refined_on_device() == key
        out.append((p.forest_cells(), p.forest_parents(), p.closed_flags(), p.vector("solution")))
        p.close()
    a, b = out
    rc.same_forest(a[0], b[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(bits(a[3]), bits(b[3]))


def test_host_cycle_keeps_the_host_loops(golden_dir):
    """cycles that do not run on the device: one line says why, the refinement is the host's"""
    p = golden_make(golden_dir, "atom_n1_8.data", 1.0, 2, "SSOR")(True)
    q = golden_make(golden_dir, "atom_n1_8.data", 1.0, 2, "SSOR")(False)
    for x in (p, q):
        x.run_cycle(0, on_device=False)
        x.finish_cycle_with(np.cos(np.arange(x.n_dofs())))
        x.run_cycle(1, on_device=False)
    assert not p.refined_on_device() and np.array_equal(bits(p.vector("initial_guess")), bits(q.vector("initial_guess")))
    rc.same_forest(p.forest_cells(), q.forest_cells())
    assert p.log().count("Refinement on device: not applicable (the cycle does not run on the device)") == 1
    p.close()
    q.close()


def test_distributed_run_keeps_the_host_loops(golden_dir):
    """a run on a communicator (one rank): one line says why, the result is the host path's"""
    p = golden_make(golden_dir, "atom_n1_8.data", 1.0, 2, "SSOR")(True)
    q = golden_make(golden_dir, "atom_n1_8.data", 1.0, 2, "SSOR")(False)
    p.set_communicator(0, 1, capi().Context.unique_id())
    for cycle in (0, 1):
        r1, r0 = p.run_cycle(cycle, on_device=True), q.run_cycle(cycle, on_device=True)
    assert not p.refined_on_device() and np.array_equal(bits(p.vector("initial_guess")), bits(q.vector("initial_guess")))
    assert np.array_equal(bits(p.vector("solution")), bits(q.vector("solution"))) and r1["cg_iterations"] == r0["cg_iterations"]
    assert p.log().count("Refinement on device: not applicable (the run is distributed)") == 1
    p.close()
    q.close()
