"""The end of an adaptive cycle on the resident mesh tables on the MI355X, through the C ABI:
gmg_build_face_table_resident / gmg_get_face_table, gmg_estimate_error_resident / gmg_get_marks, gmg_refine_forest_marked and
gmg_energy_norm_error_resident against their host-array siblings in a second context, on the steps and hand-built forests of
tests/refine_cases.py; the refusals and what the context holds after each; device memory over six rounds; and whole runs of the
driver with "Estimator from resident tables" off and on.  Every comparison is of bits or of integers: no tolerance."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import estimator_resident_cases as erc
import mesh_tables_reference as mtr
import refine_cases as rc
import refine_reference as rr
from gpu_util import capi, pkg
from test_coef_matrix_cpu import step16_problem
from test_estimator_resident_cpu import LINE, between_marked, sandwich_2d
from test_gpu_mesh_tables import SKIP_KEYS, norm_lines

pytestmark = pytest.mark.gpu

bits = rc.bits
STEPS_3D = [n for n in rc.STEPS if n.split(":")[0] in ("G8", "B3", "S3")]


@pytest.fixture()
def ctx():
    c = capi().Context(1)
    yield c
    c.close()


@pytest.fixture()
def two():
    """the context of the resident entries and the second one of their siblings"""
    a, b = capi().Context(1), capi().Context(1)
    yield a, b
    a.close()
    b.close()


def kw(fc, **more):
    a = dict(dim=fc.dim, n0=fc.n0, n_levels=fc.n_levels, level_ptr=fc.level_ptr, cell_coord=fc.cell_coord, cell_first_child=fc.cell_first_child)
    a.update(more)
    return a


def build(c, fc):
    """the mesh tables of the forest (first-touch numbering on every level: these tests read the tables back, whatever they are)"""
    c.build_mesh_tables(level0_lexicographic=False, **kw(fc))
    return c.get_mesh_tables()


def host_faces(fc, s=None):
    if s is not None and hasattr(s, "faces"):
        return np.asarray(s.faces[0], dtype=np.uint8), np.asarray(s.faces[1], dtype=np.int32)
    k, cell = rr.face_table(fc)
    nf, nfc = 2 * fc.dim, 1 << (fc.dim - 1)
    return np.asarray(k, dtype=np.uint8).reshape(-1, nf), np.asarray(cell, dtype=np.int32).reshape(-1, nf, nfc)


def noisy(n, seed=7):
    return np.random.default_rng(seed).standard_normal(n)


def old_solution(s, t):
    """u_old of the step in the numbering of the tables"""
    value = dict(zip((int(k) for k in s.old_vertex), s.u_old))
    return np.array([value[int(k)] for k in t.vertex_of_dof], dtype=np.float64)


def weights(nq, seed=11):
    w = np.abs(np.random.default_rng(seed + nq).standard_normal(nq)) + 0.1
    return w / w.sum()


def same_estimate(a, b, what=""):
    for k in ("eta", "kelly_sq", "residual_sq", "face_int", "mark"):
        x, y = np.ascontiguousarray(getattr(a, k)), np.ascontiguousarray(getattr(b, k))
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)
    assert np.float64(a.threshold).tobytes() == np.float64(b.threshold).tobytes() and a.n_marked == b.n_marked, (what, a.threshold, b.threshold)


def estimates(c, c2, fc, t, faces, u, ng, residual, nq, dens_on_device, fraction=0.6):
    """(resident estimate, sibling's estimate in the second context) of one configuration"""
    T = erc.level_tables(fc.dim, 1.0, ng, 1)
    w = weights(nq)
    dens = None
    dens_on_device = dens_on_device and t.n_cells > 0   # (no cells: nothing to leave there)
    if residual:
        rng = np.random.default_rng(3)
        if dens_on_device:   # densities left on the device by gmg_charge_density, at any points: only their shape and bits matter here
            lo = rng.uniform(0.0, 1.0, (t.n_cells, 3))
            c.charge_density(lo, np.full(t.n_cells, 0.5), np.floor(lo), 1.0, rng.uniform(0, 1, (3, 3)), np.array([1.0, -1.0, 0.5]), 0.5, 10.0, False,
                             rng.uniform(0, 1, (nq, 3)), dens=None)
            dens = c.get_charge_density(t.n_cells, nq)
            assert t.n_cells == 0 or np.abs(dens).max() > 0
        else:
            dens = np.abs(rng.standard_normal((t.n_cells, nq))) * 0.05
    v, v2 = c.vector(max(len(u), 1), u if len(u) else None), c2.vector(max(len(u), 1), u if len(u) else None)
    try:
        common = dict(residual=residual, weight=w if residual else None, jxw_of_level=T.jxw_of_level if residual else None, fraction=fraction, n_u=len(u))
        res = c.estimate_error_resident(T.h_of_level, T.face_measure_of_level, T.diameter_of_level, T.gauss_x, T.gauss_w, v,
                                        dens=None if dens_on_device else dens, dim=fc.dim, **common)
        sib = c2.estimate_error(fc.dim, t.cell_dofs, t.cell_level, faces[0], faces[1], T.h_of_level, T.face_measure_of_level, T.diameter_of_level,
                                T.gauss_x, T.gauss_w, v2, dens=dens, **common)
    finally:
        v.free()
        v2.free()
    return res, sib


# ------------------------------------------------------------------------------------------------ 1. the face table

def check_face_table(c, fc, faces, what):
    first = None
    for max_blocks in (0, 1, 3):   # by size; one workgroup; three (every grid-stride loop iterates)
        c.set_option("assemble_max_blocks", max_blocks)
        t = build(c, fc)
        r = c.build_face_table_resident(**kw(fc))
        got, plain = c.get_face_table(), c.build_face_table(**kw(fc))
        assert r.n_active == got.n_active == plain.n_active == t.n_cells == len(faces[0]), (what, max_blocks)
        assert np.array_equal(got.face_kind, faces[0]) and np.array_equal(got.face_cell, faces[1]), (what, max_blocks)
        assert np.array_equal(got.face_kind, plain.face_kind) and np.array_equal(got.face_cell, plain.face_cell), (what, max_blocks)
        first = first or got
        assert np.array_equal(first.face_kind, got.face_kind) and np.array_equal(first.face_cell, got.face_cell)
    c.set_option("assemble_max_blocks", 0)


@pytest.mark.parametrize("name", rc.STEPS)
def test_face_table_equals_the_host_s(ctx, name):
    s = rc.step(name)
    check_face_table(ctx, s.fc, host_faces(s.fc, s), name)
    check_face_table(ctx, s.new_fc, (np.asarray(s.new_faces[0]), np.asarray(s.new_faces[1])), name + " (new)")


@pytest.mark.parametrize("name", sorted(rc.HAND_BUILT) + ["sandwich-2d"])
def test_face_table_of_hand_built_forests(ctx, name):
    fc = sandwich_2d()[0] if name == "sandwich-2d" else rc.hand(name).fc
    check_face_table(ctx, fc, host_faces(fc), name)


def test_two_face_tables_in_a_row(ctx):
    x, y = rc.step("G8:0->1"), rc.step("B3:0->1")
    build(ctx, x.fc)
    ctx.build_face_table_resident(**kw(x.fc))
    build(ctx, y.fc)                                   # new tables: the face table went with the old ones
    with pytest.raises(capi().GMGError):
        ctx.get_face_table()
    ctx.build_face_table_resident(**kw(y.fc))
    ctx.build_face_table_resident(**kw(y.fc))
    got, want = ctx.get_face_table(), host_faces(y.fc, y)
    assert np.array_equal(got.face_kind, want[0]) and np.array_equal(got.face_cell, want[1])


# ------------------------------------------------------------------------------------------------ 2. the estimator and the marks

#  (u, ng, residual, nq, densities on the device): every value of the issue's lists occurs
CONFIGS = [("old", 2, 0, 1, False), ("noisy", 1, 1, 1, False), ("noisy", 2, 1, 8, True), ("old", 3, 2, 27, False), ("noisy", 3, 2, 8, True),
           ("old", 1, 1, 27, True)]


@pytest.mark.parametrize("name", rc.STEPS)
def test_estimate_equals_the_sibling_s(two, name):
    c, c2 = two
    s = rc.step(name)
    t = build(c, s.fc)
    c.build_face_table_resident(**kw(s.fc))
    faces = host_faces(s.fc, s)
    partial = False
    for which, ng, residual, nq, on_device in CONFIGS:
        u = old_solution(s, t) if which == "old" else noisy(t.n_dofs)
        first = None
        for max_blocks in (0, 1, 3):
            c.set_option("estimate_max_blocks", max_blocks)
            res, sib = estimates(c, c2, s.fc, t, faces, u, ng, residual, nq, on_device)
            same_estimate(res, sib, (name, which, ng, residual, nq, on_device, max_blocks))
            m = c.get_marks()
            assert m.n_cells == t.n_cells and m.n_marked == res.n_marked == int(res.mark.sum()) and np.array_equal(m.mark, res.mark)
            first = first or res
            same_estimate(first, res, (name, "launch shape", max_blocks))
        partial |= 0 < res.n_marked < t.n_cells
        assert np.abs(res.face_int).max() > 0 and (not residual or np.abs(res.residual_sq).max() > 0)
    assert partial, name


@pytest.mark.parametrize("name", sorted(rc.HAND_BUILT) + ["sandwich-2d"])
def test_estimate_on_hand_built_forests(two, name):
    c, c2 = two
    fc = sandwich_2d()[0] if name == "sandwich-2d" else rc.hand(name).fc
    t = build(c, fc)
    c.build_face_table_resident(**kw(fc))
    for ng, residual, nq, on_device in ((2, 0, 1, False), (3, 1, 8, True), (1, 2, 27, False)):
        res, sib = estimates(c, c2, fc, t, host_faces(fc), noisy(t.n_dofs), ng, residual, nq, on_device)
        same_estimate(res, sib, (name, ng, residual, nq))
        m = c.get_marks()
        assert m.n_cells == t.n_cells and m.n_marked == res.n_marked and np.array_equal(m.mark, res.mark)
    if t.n_cells == 0:
        assert res.threshold == 0.0 and res.n_marked == 0


# ------------------------------------------------------------------------------------------------ 3. the refinement from the marks

def same_refinement(c, c2, fc, what, restate=True):
    """gmg_refine_forest_marked on the marks c holds against gmg_refine_forest fed the restatement's flags from the same marks"""
    m = c.get_marks()
    flag = erc.flags_from_marks(fc, m.mark)
    r = c.refine_forest_marked(**kw(fc))
    got = c.get_refined_forest()
    r2 = c2.refine_forest(flag=flag if len(flag) else None, **kw(fc))
    want = c2.get_refined_forest()
    assert (r.n_levels, r.n_cells, r.n_split) == (r2.n_levels, r2.n_cells, r2.n_split) == (got.n_levels, got.n_cells, got.n_split), what
    for k in ("level_ptr", "cell_coord", "cell_first_child", "cell_parent", "closed_flag"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), (what, k)
    if restate:   # and the restatement of the closure and the split
        ref = rr.refine(fc, flag.tolist())
        assert np.array_equal(got.closed_flag, np.asarray(ref.closed_flag, dtype=np.uint8)) and got.n_split == ref.n_split, what
    after = c.get_marks()                # the marks are left in place
    assert np.array_equal(after.mark, m.mark) and after.n_marked == m.n_marked
    return flag, got


@pytest.mark.parametrize("name", rc.STEPS)
def test_refinement_from_the_marks(two, name):
    c, c2 = two
    s = rc.step(name)
    t = build(c, s.fc)
    c.build_face_table_resident(**kw(s.fc))
    faces = host_faces(s.fc, s)
    grows = False
    for u, fraction in ((old_solution(s, t), 0.6), (noisy(t.n_dofs), 0.5), (noisy(t.n_dofs, 8), 0.9)):
        res, _ = estimates(c, c2, s.fc, t, faces, u, 2, 0, 1, False, fraction=fraction)
        for max_blocks in (0, 1, 3):
            c.set_option("assemble_max_blocks", max_blocks)
            flag, got = same_refinement(c, c2, s.fc, (name, fraction, max_blocks), restate=max_blocks == 0 and fraction == 0.5)
        grows |= bool((got.closed_flag > flag).any())
        assert 0 < res.n_marked
    # the step's own marks give the step's own closure (the marks of the host's estimate, where the device's equal them)
    res, _ = estimates(c, c2, s.fc, t, faces, old_solution(s, t), 2, 0, 1, False)
    if np.array_equal(erc.flags_from_marks(s.fc, res.mark), np.asarray(s.flag, dtype=np.uint8)):
        _, got = same_refinement(c, c2, s.fc, name, restate=False)   # (the host's own closure stands for it)
        assert np.array_equal(got.closed_flag, np.asarray(s.closed, dtype=np.uint8))
        rc.same_forest(got, s.new_fc, name)
    print(f"{name}: the closure added flags in some round: {grows}")


@pytest.mark.parametrize("name", sorted(rc.HAND_BUILT) + ["sandwich-2d"])
def test_refinement_of_hand_built_forests(two, name):
    """no-flags, inactive-only and zero-cells with no mark at all (a fraction above 1 marks nothing); the others with some"""
    c, c2 = two
    fc = sandwich_2d()[0] if name == "sandwich-2d" else rc.hand(name).fc
    t = build(c, fc)
    c.build_face_table_resident(**kw(fc))
    none = name in ("no-flags", "inactive-only", "zero-cells")
    for seed in (1, 2, 3):
        res, _ = estimates(c, c2, fc, t, host_faces(fc), noisy(t.n_dofs, seed), 2, 0, 1, False, fraction=2.0 if none else 0.5)
        assert (res.n_marked == 0) == (none or t.n_cells == 0), (name, res.n_marked)
        flag, got = same_refinement(c, c2, fc, (name, seed))
        if none:
            assert got.n_split == 0 and not got.closed_flag.any()
    if name == "sandwich-2d":   # every active cell marked: the inactive cell between them must stay unflagged
        res, _ = estimates(c, c2, fc, t, host_faces(fc), noisy(t.n_dofs), 2, 0, 1, False, fraction=0.0)
        assert res.n_marked == t.n_cells
        flag, got = same_refinement(c, c2, fc, name)
        assert between_marked(fc, flag) and flag.sum() == t.n_cells and not flag[np.asarray(fc.cell_first_child) >= 0].any()


# ------------------------------------------------------------------------------------------------ 4. the error norm

def norm_inputs(nq, n_atoms, seed=5):
    rng = np.random.default_rng(seed + nq + n_atoms)
    return SimpleNamespace(qp=rng.uniform(0.05, 0.95, (nq, 3)), w=weights(nq), sg=rng.standard_normal((nq, 8, 3)),
                           xyz=rng.uniform(0.0, 1.0, (n_atoms, 3)), q=rng.choice([-1.0, 1.0], n_atoms))


@pytest.mark.parametrize("name", STEPS_3D)
def test_error_norm_equals_the_sibling_s(two, name):
    c, c2 = two
    s = rc.step(name)
    assert s.fc.dim == 3
    t = build(c, s.fc)
    u = old_solution(s, t)
    v, v2 = c.vector(len(u), u), c2.vector(len(u), u)
    for origin, h0 in ((0.0, 1.0), (-0.375, 0.3)):
        lo, hh, _ = c.get_resident_cell_geometry(origin, h0, want=(True, True, False))
        for nq, n_atoms in ((1, 40), (8, 0), (8, 1), (27, 40), (64, 40), (64, 1)):
            i = norm_inputs(nq, n_atoms)
            xyz = origin + i.xyz * h0 * max(s.fc.n0)
            err, ce = c.energy_norm_error_resident(origin, h0, v, xyz, i.q, 0.4 * h0, i.qp, i.w, i.sg)
            err2, ce2 = c2.energy_norm_error(lo, hh, t.cell_dofs, v2, xyz, i.q, 0.4 * h0, i.qp, i.w, i.sg)
            assert np.float64(err).tobytes() == np.float64(err2).tobytes() and np.array_equal(bits(ce), bits(ce2)), (name, origin, nq, n_atoms)
            assert err > 0 and ce.shape == (t.n_cells,)
    v.free()
    v2.free()


# ------------------------------------------------------------------------------------------------ 5. refusals, and what is held

def changed(fc, **more):
    d = dict(vars(fc))
    d.update(more)
    return SimpleNamespace(**d)


def refused(code, call, text=None):
    with pytest.raises(capi().GMGError) as e:
        call()
    assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)
    return True


def holds(c):
    """(a face table is held, marks are held)"""
    out = []
    for get in (c.get_face_table, c.get_marks):
        try:
            get()
            out.append(True)
        except capi().GMGError as e:
            assert e.code == capi().ERR_INVALID
            out.append(False)
    return tuple(out)


def plain_estimate(c, fc, n_dofs, **change):
    T = erc.level_tables(fc.dim, 1.0, 2, 1)
    a = dict(h_of_level=T.h_of_level, face_measure_of_level=T.face_measure_of_level, diameter_of_level=T.diameter_of_level, gauss_x=T.gauss_x,
             gauss_w=T.gauss_w, residual=0, weight=None, jxw_of_level=None, dens=None, fraction=0.5, n_u=n_dofs, dim=fc.dim)
    a.update(change)
    v = c.vector(max(n_dofs, 1), noisy(n_dofs) if n_dofs else None)
    try:
        return c.estimate_error_resident(u=v, **a)
    finally:
        v.free()


def test_refusals_of_the_face_table(ctx):
    A = capi()
    s = rc.hand("staircase-2d")
    fc = s.fc
    assert refused(A.ERR_INVALID, lambda: ctx.build_face_table_resident(**kw(fc)), "no mesh tables")
    assert refused(A.ERR_INVALID, ctx.get_face_table, "no face table")
    t = build(ctx, fc)
    assert refused(A.ERR_INVALID, ctx.get_face_table, "no face table")
    twice = changed(fc, cell_coord=fc.cell_coord[:5] + [fc.cell_coord[4]] + fc.cell_coord[6:])
    bad = [(A.ERR_INVALID, changed(fc, dim=4), None), (A.ERR_INVALID, changed(fc, cell_coord=None), None),
           (A.ERR_INVALID, rc.hand("single-3d").fc, "dim differs"), (A.ERR_INVALID, rc.hand("lattice-2x2").fc, "active cells"),
           (A.ERR_INVALID, twice, "appears twice")]
    for code, other, text in bad:
        ctx.build_face_table_resident(**kw(fc))
        plain_estimate(ctx, fc, t.n_dofs)
        assert holds(ctx) == (True, True)
        assert refused(code, lambda: ctx.build_face_table_resident(**kw(other)), text)
        assert holds(ctx) == (False, False), text       # no face table after a failed build (and no marks formed with the old one)
        assert ctx.get_mesh_tables().n_cells == t.n_cells   # the tables themselves stay
    ctx.build_face_table_resident(**kw(fc))
    assert holds(ctx) == (True, False)


def test_refusals_of_the_estimate(ctx):
    A = capi()
    fc = rc.hand("staircase-2d").fc
    assert refused(A.ERR_INVALID, lambda: plain_estimate(ctx, fc, 10), "no mesh tables")
    assert refused(A.ERR_INVALID, ctx.get_marks, "no marks")
    t = build(ctx, fc)
    assert refused(A.ERR_INVALID, lambda: plain_estimate(ctx, fc, t.n_dofs), "no face table")
    ctx.build_face_table_resident(**kw(fc))
    T = erc.level_tables(2, 1.0, 2, 1)
    w = weights(4)
    ctx.charge_density(np.zeros((t.n_cells, 3)), np.ones(t.n_cells), np.zeros((t.n_cells, 3)), 1.0, np.full((1, 3), 0.5), np.ones(1), 0.5, 10.0, False,
                       np.full((8, 3), 0.5), dens=None)   # device densities of n_cells x 8
    bad = [("n_dofs", dict(n_u=t.n_dofs + 1)), ("n_dofs", dict(n_u=t.n_dofs - 1)), ("ng", dict(gauss_x=np.zeros(0), gauss_w=np.zeros(0))),
           ("ng", dict(gauss_x=np.zeros(9), gauss_w=np.zeros(9))), ("residual", dict(residual=3)), ("fraction", dict(fraction=-1.0)),
           ("fraction", dict(fraction=float("nan"))), ("nq", dict(residual=1, weight=np.zeros(0), jxw_of_level=T.jxw_of_level)),
           ("NULL", dict(h_of_level=None)), ("NULL", dict(residual=2, weight=w, jxw_of_level=None, dens=np.ones((t.n_cells, 4)))),
           ("densities", dict(residual=1, weight=w, jxw_of_level=T.jxw_of_level, dens=None))]   # on the device: n_cells x 8, not x 4
    for text, change in bad:
        plain_estimate(ctx, fc, t.n_dofs)
        assert holds(ctx) == (True, True)
        assert refused(A.ERR_INVALID, lambda: plain_estimate(ctx, fc, t.n_dofs, **change), text)
        assert holds(ctx) == (True, False), text        # no marks after a failed estimate; the face table stays
    ctx.charge_density(np.zeros((1, 3)), np.ones(1), np.zeros((1, 3)), 1.0, np.full((1, 3), 0.5), np.ones(1), 0.5, 10.0, False, np.full((4, 3), 0.5), dens=True)
    assert refused(A.ERR_INVALID, lambda: plain_estimate(ctx, fc, t.n_dofs, residual=1, weight=w, jxw_of_level=T.jxw_of_level, dens=None), "densities")   # none left
    ok = plain_estimate(ctx, fc, t.n_dofs, residual=1, weight=w, jxw_of_level=T.jxw_of_level, dens=np.ones((t.n_cells, 4)))
    assert holds(ctx) == (True, True) and ok.n_marked > 0


def test_refusals_of_the_refinement(ctx):
    A = capi()
    s = rc.hand("staircase-2d")
    fc = s.fc
    assert refused(A.ERR_INVALID, lambda: ctx.refine_forest_marked(**kw(fc)), "no mesh tables")
    t = build(ctx, fc)
    ctx.build_face_table_resident(**kw(fc))
    assert refused(A.ERR_INVALID, lambda: ctx.refine_forest_marked(**kw(fc)), "no marks")
    ctx.refine_forest(flag=s.flag, **kw(fc))            # something to lose
    before = ctx.get_refined_forest()
    plain_estimate(ctx, fc, t.n_dofs)
    marks = ctx.get_marks()
    twice = changed(fc, cell_coord=fc.cell_coord[:5] + [fc.cell_coord[4]] + fc.cell_coord[6:])
    for code, other, text in ((A.ERR_INVALID, rc.hand("lattice-2x2").fc, "active cells"), (A.ERR_INVALID, changed(fc, dim=4), None),
                              (A.ERR_INVALID, changed(fc, cell_first_child=None), None), (A.ERR_INVALID, twice, "appears twice"),
                              (A.ERR_INVALID, changed(fc, n0=(0, 4, 1)), None)):
        assert refused(code, lambda: ctx.refine_forest_marked(**kw(other)), text)
        after, m = ctx.get_refined_forest(), ctx.get_marks()     # the marks untouched, the refined forest what it was
        assert np.array_equal(m.mark, marks.mark) and m.n_marked == marks.n_marked and holds(ctx) == (True, True)
        for k, v in vars(before).items():
            assert np.array_equal(v, getattr(after, k)), k
    deep = rr.corner_12()                                # a mark on level 12: no level beyond it, as in the sibling
    td = build(ctx, deep)
    ctx.build_face_table_resident(**kw(deep))
    assert plain_estimate(ctx, deep, td.n_dofs, fraction=0.0).n_marked == td.n_cells
    assert refused(A.ERR_UNSUPPORTED, lambda: ctx.refine_forest_marked(**kw(deep)), "level 12")
    assert holds(ctx) == (True, True)


def test_refusals_of_the_error_norm(ctx):
    A = capi()
    s = rc.step("G8:0->1")
    i = norm_inputs(8, 3)
    v = ctx.vector(10, noisy(10))
    call = lambda u=None, origin=0.0, h0=1.0, r_c=0.5, i=i, n_u=None: ctx.energy_norm_error_resident(origin, h0, u or v, i.xyz, i.q, r_c, i.qp, i.w, i.sg, n_u=n_u)
    assert refused(A.ERR_INVALID, call, "no mesh tables")
    t = build(ctx, s.fc)
    u = ctx.vector(t.n_dofs, noisy(t.n_dofs))
    assert refused(A.ERR_INVALID, lambda: call(u, h0=0.0), "h0") and refused(A.ERR_INVALID, lambda: call(u, h0=-1.0), "h0")
    assert refused(A.ERR_INVALID, lambda: call(v), "n_dofs") and refused(A.ERR_INVALID, lambda: call(u, n_u=t.n_dofs + 1), "n_dofs")
    assert refused(A.ERR_INVALID, lambda: call(u, r_c=0.0)) and refused(A.ERR_UNSUPPORTED, lambda: call(u, i=norm_inputs(65, 3)), "64")
    assert call(u)[0] > 0
    build(ctx, rc.hand("staircase-2d").fc)
    assert refused(A.ERR_UNSUPPORTED, lambda: call(u), "3D")
    build(ctx, mtr.empty(3))
    assert ctx.energy_norm_error_resident(0.0, 1.0, v, i.xyz, i.q, 0.5, i.qp, i.w, i.sg, n_u=0)[0] == 0.0   # zero cells
    u.free()
    v.free()


def test_unsupported_on_a_communicator():
    A = capi()
    c = A.Context(1)
    fc = rc.hand("staircase-2d").fc
    c.comm_init(0, 1, A.Context.unique_id())
    i = norm_inputs(8, 3)
    v = c.vector(10, noisy(10))
    for call in (lambda: c.build_face_table_resident(**kw(fc)), c.get_face_table, lambda: plain_estimate(c, fc, 10), c.get_marks,
                 lambda: c.refine_forest_marked(**kw(fc)), lambda: c.energy_norm_error_resident(0.0, 1.0, v, i.xyz, i.q, 0.5, i.qp, i.w, i.sg)):
        assert refused(A.ERR_UNSUPPORTED, call, "communicator")
    v.free()
    c.close()


def test_reset_with_and_without_the_tables_kept(ctx):
    A = capi()
    fc = rc.hand("staircase-2d").fc
    for keep in (1, 0):
        t = build(ctx, fc)
        ctx.build_face_table_resident(**kw(fc))
        plain_estimate(ctx, fc, t.n_dofs)
        faces, marks = ctx.get_face_table(), ctx.get_marks()
        ctx.set_option("reset_keeps_mesh_tables", keep)
        assert ctx.L.gmg_reset(ctx.h, C.c_int(2)) == A.OK
        ctx.set_option("reset_keeps_mesh_tables", 0)
        assert holds(ctx) == (bool(keep), bool(keep))
        if keep:
            assert np.array_equal(ctx.get_face_table().face_cell, faces.face_cell) and np.array_equal(ctx.get_marks().mark, marks.mark)
            assert ctx.refine_forest_marked(**kw(fc)).n_split > 0
        else:
            assert refused(A.ERR_INVALID, lambda: ctx.refine_forest_marked(**kw(fc)), "no mesh tables")
    t = build(ctx, fc)   # and a new build drops both
    ctx.build_face_table_resident(**kw(fc))
    plain_estimate(ctx, fc, t.n_dofs)
    build(ctx, fc)
    assert holds(ctx) == (False, False)


def test_no_leak_over_six_rounds():
    """as tests/test_gpu_lifecycle.py: build, face table, estimate, refine, error norm, reset, six times in one context; the free
    device memory after the last round equals that after the first"""
    import torch

    s = rc.step("B3:0->1")
    i = norm_inputs(8, 5)
    c = capi().Context(1)
    free = []
    for _ in range(6):
        t = build(c, s.fc)
        c.build_face_table_resident(**kw(s.fc))
        assert plain_estimate(c, s.fc, t.n_dofs).n_marked > 0
        assert c.refine_forest_marked(**kw(s.fc)).n_split > 0
        v = c.vector(t.n_dofs, noisy(t.n_dofs))
        assert c.energy_norm_error_resident(0.0, 1.0, v, i.xyz, i.q, 0.5, i.qp, i.w, i.sg)[0] > 0
        v.free()
        assert c.L.gmg_reset(c.h, C.c_int(1)) == capi().OK
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    c.close()
    print("free device memory after each round, relative to the first:", [f - free[0] for f in free])
    assert free[-1] == free[0], free


# ------------------------------------------------------------------------------------------------ 6. whole runs of the driver

ALL_KEYS = dict(mesh_tables_on_device=True, system_matrix_on_device=True, level_matrices_on_device=True, rhs_from_cell_tables=True,
                operators_from_resident_tables=True, estimator_on_device=True, analytical_on_device=True, refinement_on_device=True, transfer_on_device=True)


def golden_problem(name, right, cycles, vacuum, key, **more):
    S = pkg().step50
    args = dict(ALL_KEYS, densities_from_resident_tables=True)
    args.update(more)
    p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=vacuum, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=cycles, r_c=0.5,
                             cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR", estimator_from_resident_tables=key, **args))
    p.read_lammps(os.path.join(rc.mtc.GOLDEN, name))
    return p


def driver_runs(make, cycles, lammps):
    """the same run with the key off and on, the driver holding the device's face table and flags against its own
    (STEP50_CHECK_RESIDENT): everything but the times must be equal"""
    runs = {}
    for key in (False, True):
        p = make(key)
        out = []
        for cycle in range(cycles):
            rep = p.run_cycle(cycle, on_device=True)
            assert p.estimator_resident() == key and p.operators_resident() and p.estimated_on_device(), (key, cycle)
            assert p.refined_on_device() == (cycle > 0)
            norm = p.cell_errors(on_device=True, norm=True) if lammps else (np.zeros(0), 0.0)
            out.append((rep, p.marks(), p.refine_flags(), p.error_per_cell(), p.vector("solution"), p.vector("initial_guess"), p.forest_cells(),
                        p.closed_flags(), p.face_integrals(), norm))
        assert "Estimator from resident tables" not in p.log(), p.log()   # no fallback line
        runs[key] = (out, norm_lines(p.log()))
        p.close()
    assert runs[False][1] == runs[True][1]
    for cycle, (a, b) in enumerate(zip(runs[False][0], runs[True][0])):
        for k in a[0]:
            if k not in SKIP_KEYS:   # counts, thresholds, iteration counts, norms; the energy-norm error is the device's fixed-order sum here
                assert repr(a[0][k]) == repr(b[0][k]), (cycle, k, a[0][k], b[0][k])
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[7], b[7]), cycle
        assert a[3].tobytes() == b[3].tobytes(), cycle
        for i in (4, 5, 8):
            assert np.array_equal(bits(a[i]), bits(b[i])), (cycle, i)
        for k in ("n_levels", "level_ptr", "cell_coord", "cell_first_child"):
            assert np.array_equal(getattr(a[6], k), getattr(b[6], k)), (cycle, k)
        assert np.array_equal(bits(a[9][0]), bits(b[9][0])) and np.float64(a[9][1]).tobytes() == np.float64(b[9][1]).tobytes(), cycle
    return runs


@pytest.mark.parametrize("name,right,cycles,vacuum,estimator", [("atom_n1_8.data", 1.0, 3, 10, "Kelly + residual"), ("atom_n1_8.data", 1.0, 3, 10, "Kelly"),
                                                                 ("atom_n3_216.data", 3.0, 2, 2, "Kelly")],
                         ids=["8-atoms-3-cycles-residual", "8-atoms-3-cycles-kelly", "216-atoms-2-cycles"])
def test_driver_runs_with_the_key_off_and_on(name, right, cycles, vacuum, estimator, monkeypatch):
    monkeypatch.setenv("STEP50_CHECK_RESIDENT", "1")
    runs = driver_runs(lambda key: golden_problem(name, right, cycles, vacuum, key, refinement_estimator=estimator), cycles, True)
    last = runs[True][0][-1]
    assert last[0]["cg_iterations"] >= 1 and len(last[0]["dofs_by_level"]) >= 2 and 0 < last[1].sum() < len(last[1]) and last[9][1] > 0


@pytest.mark.parametrize("dim,refine_times", ((2, 3), (3, 2)))
def test_step16_runs_with_the_key_off_and_on(dim, refine_times, monkeypatch):
    monkeypatch.setenv("STEP50_CHECK_RESIDENT", "1")
    runs = driver_runs(lambda key: step16_problem(dim, refine_times, 3, estimator_from_resident_tables=key, **ALL_KEYS), 3, False)
    assert len(runs[True][0][-1][0]["dofs_by_level"]) >= refine_times + 2


@pytest.mark.parametrize("missing,why", [("operators_from_resident_tables", "Operators from resident tables did not take effect"),
                                         ("estimator_on_device", "Error estimator on device is not set"),
                                         ("refinement_on_device", "Refinement on device is not set")])
def test_a_missing_prerequisite_keeps_the_host_arrays(missing, why):
    """one line says why, once over two cycles, and the run is the one without the key"""
    p, q = (golden_problem("atom_n1_8.data", 1.0, 2, 2, key, refinement_estimator="Kelly", **{missing: False}) for key in (True, False))
    for cycle in range(2):
        r1, r0 = p.run_cycle(cycle, on_device=True), q.run_cycle(cycle, on_device=True)
        assert not p.estimator_resident() and r1["cg_iterations"] == r0["cg_iterations"] and repr(r1["refine_threshold"]) == repr(r0["refine_threshold"])
        assert np.array_equal(p.marks(), q.marks()) and np.array_equal(bits(p.vector("solution")), bits(q.vector("solution")))
        assert p.error_per_cell().tobytes() == q.error_per_cell().tobytes()
    assert p.log().count(LINE.format(why)) == 1 and "Estimator from resident tables" not in q.log()
    p.close()
    q.close()


def test_a_distributed_run_keeps_the_host_arrays():
    p, q = (golden_problem("atom_n1_8.data", 1.0, 2, 2, key, refinement_estimator="Kelly") for key in (True, False))
    p.set_communicator(0, 1, capi().Context.unique_id())
    for cycle in range(2):
        r1, r0 = p.run_cycle(cycle, on_device=True), q.run_cycle(cycle, on_device=True)
        assert not p.estimator_resident() and r1["cg_iterations"] == r0["cg_iterations"]
        assert np.array_equal(p.marks(), q.marks())
    assert p.log().count(LINE.format("the run is distributed")) == 1
    p.close()
    q.close()


def test_refine_with_flags_takes_the_caller_s_flags():
    """Problem.refine_with_flags after a resident estimate: the flags that are passed count, not the marks the context holds"""
    out = []
    for key in (False, True):
        p = golden_problem("atom_n1_8.data", 1.0, 2, 2, key, refinement_estimator="Kelly")
        p.run_cycle(0, on_device=True)
        assert p.estimator_resident() == key
        flags = p.refine_flags()
        flags[::7] = 1
        p.refine_with_flags(flags, on_device=True)
        assert p.refined_on_device()
        out.append((p.forest_cells(), p.closed_flags(), p.vector("solution")))
        p.close()
    a, b = out
    rc.same_forest(a[0], b[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))
