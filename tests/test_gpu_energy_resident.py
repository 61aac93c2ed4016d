"""Energy and forces at the atoms on the resident mesh tables on the MI355X, through the C ABI:
gmg_build_point_locator_resident / gmg_get_point_locator against the plain-numpy restatement and the host's array,
gmg_atom_forces_resident against gmg_atom_forces in a second context fed the downloaded tables and that array,
gmg_electrostatic_energy_resident against the plain-Python sums of the sibling's per-atom values and against the mpmath and numpy
references of tests/atoms_reference.py; the refusals and what the context holds after each; device memory over six rounds; and
whole runs of the driver with "Energy and forces from resident tables" off and on.  Comparisons are of bits or integers; the one
tolerance is the derived bound of the short-range sum (tests/energy_resident_cases.py)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import energy_resident_cases as erc
import mesh_tables_reference as mtr
import refine_cases as rc
from gpu_util import capi, pkg
from test_coef_matrix_cpu import step16_problem
from test_energy_resident_cpu import LINE

pytestmark = pytest.mark.gpu

bits = rc.bits
STEPS_3D = [n for n in rc.STEPS if n.split(":")[0] in ("G8", "B3", "S3")]
KEYS = ("phi", "field", "force", "force_short", "e_short")


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


def changed(fc, **more):
    d = dict(vars(fc))
    d.update(more)
    return SimpleNamespace(**d)


def build(c, fc):
    c.build_mesh_tables(level0_lexicographic=False, **kw(fc))
    return c.get_mesh_tables()


def refused(code, call, text=None):
    with pytest.raises(capi().GMGError) as e:
        call()
    assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)
    return True


def holds(c):
    """is a resident locator held?"""
    try:
        c.get_point_locator()
        return True
    except capi().GMGError as e:
        assert e.code == capi().ERR_INVALID
        return False


def noisy(n, seed=7):
    return np.random.default_rng(seed).standard_normal(n)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ 1. the locator

def check_locator(c, fc, want, what):
    for max_blocks in (0, 1, 3):   # by size; one workgroup; three (the grid-stride loop iterates)
        c.set_option("assemble_max_blocks", max_blocks)
        t = build(c, fc)
        r = c.build_point_locator_resident(**kw(fc))
        got = c.get_point_locator()
        assert r.n_nodes == len(got) == len(want) and got.dtype == np.int32, (what, max_blocks)
        assert np.array_equal(got, want), (what, max_blocks)
        assert (got < 0).sum() == t.n_cells
    c.set_option("assemble_max_blocks", 0)


@pytest.mark.parametrize("name", STEPS_3D)
def test_locator_equals_the_restatement_and_the_host_s(ctx, name):
    fc, node, new_fc, new_node = erc.host_nodes(name)
    for f, host in ((fc, node), (new_fc, new_node)):
        want = erc.node_array(f)
        assert np.array_equal(want, host)
        check_locator(ctx, f, want, name)


@pytest.mark.parametrize("name", sorted(erc.FORESTS) + ["single-3d", "empty-3d"])
def test_locator_of_hand_built_forests(ctx, name):
    fc = {"single-3d": lambda: mtr.single_cell(3), "empty-3d": lambda: mtr.empty(3)}.get(name, lambda: erc.forest(name))()
    check_locator(ctx, fc, erc.node_array(fc), name)


def test_refusals_of_the_locator(ctx):
    """what the context holds after each refusal: no resident locator (the call drops the held one first), the mesh tables
    untouched"""
    A = capi()
    fc = erc.forest("deep")
    assert refused(A.ERR_INVALID, lambda: ctx.build_point_locator_resident(**kw(fc)), "no mesh tables")
    assert refused(A.ERR_INVALID, ctx.get_point_locator, "no mesh tables")
    t = build(ctx, fc)
    assert refused(A.ERR_INVALID, ctx.get_point_locator, "no point locator")
    cc = np.asarray(fc.cell_coord, dtype=np.int32).reshape(-1, 3)
    swapped = cc.copy()
    swapped[[0, 1]] = swapped[[1, 0]]        # the first two roots change places: still a valid forest, not lexicographic
    cases = ((A.ERR_INVALID, rc.hand("staircase-2d").fc, "dim differs"),               # a wrong dim (a valid 2D forest: the tables' is 3)
             (A.ERR_INVALID, changed(fc, dim=4), None),                                # the sibling's forest checks with its codes
             (A.ERR_INVALID, changed(fc, cell_first_child=None), None),
             (A.ERR_INVALID, erc.forest("wide"), "active cells"),                      # a wrong active count
             (A.ERR_INVALID, changed(fc, cell_coord=swapped), "lexicographic"),        # a level 0 out of order
             (A.ERR_INVALID, changed(erc.forest("lattice-2"), n0=[2, 2, 3]), None))    # a level 0 that is not the full lattice
    for code, other, text in cases:
        ctx.build_point_locator_resident(**kw(fc))
        assert holds(ctx)
        assert refused(code, lambda: ctx.build_point_locator_resident(**kw(other)), text)
        assert not holds(ctx)
        again = ctx.get_mesh_tables()
        assert again.n_cells == t.n_cells and np.array_equal(again.cell_dofs, t.cell_dofs)
    lat = erc.forest("lattice-2")
    build(ctx, lat)
    assert refused(A.ERR_INVALID, lambda: ctx.build_point_locator_resident(**kw(changed(lat, n0=[2, 2, 3]))), "full lattice")
    # forces and energy without a locator, and with bad arguments
    v = ctx.vector(27, noisy(27))
    xyz, q = erc.atom_set(lat, 0.0, 1.0, 1)
    assert refused(A.ERR_INVALID, lambda: ctx.atom_forces_resident(0.0, 1.0, xyz, q, v, 0.5), "no point locator")
    assert refused(A.ERR_INVALID, lambda: ctx.electrostatic_energy_resident(0.0, 1.0, xyz, q, v, 0.5), "no point locator")
    ctx.build_point_locator_resident(**kw(lat))
    for call in (ctx.atom_forces_resident, ctx.electrostatic_energy_resident):
        assert refused(A.ERR_INVALID, lambda: call(0.0, 0.0, xyz, q, v, 0.5), "h0") and refused(A.ERR_INVALID, lambda: call(0.0, -1.0, xyz, q, v, 0.5), "h0")
        assert refused(A.ERR_INVALID, lambda: call(0.0, 1.0, xyz, q, v, 0.5, n_u=26), "n_dofs") and refused(A.ERR_INVALID, lambda: call(0.0, 1.0, xyz, q, v, 0.5, n_u=28), "n_dofs")
        assert refused(A.ERR_INVALID, lambda: call(0.0, 1.0, xyz, q, v, 0.0)) and refused(A.ERR_INVALID, lambda: call(0.0, 1.0, xyz, q, v, 0.5, cutoff=-1.0))
        assert holds(ctx)
    v.free()


# ------------------------------------------------------------------------------------------------ 2. the forces

@pytest.mark.parametrize("geometry", sorted(erc.GEOMETRY))
@pytest.mark.parametrize("name", sorted(erc.FORESTS))
def test_forces_equal_the_sibling_s(two, name, geometry):
    c, c2 = two
    fc = erc.forest(name)
    origin, h0 = erc.GEOMETRY[geometry]
    t = build(c, fc)
    c.build_point_locator_resident(**kw(fc))
    node = c.get_point_locator()
    assert np.array_equal(node, erc.node_array(fc))
    c2.set_point_locator(fc.n0, [origin] * 3, h0, erc.node_array(fc), t.cell_dofs)   # the downloaded tables, the host's array
    u = noisy(t.n_dofs, 11)
    v, v2 = c.vector(t.n_dofs, u), c2.vector(t.n_dofs, u)
    for n in (0, 1, 40):
        xyz, q = erc.atom_set(fc, origin, h0, n)
        for cutoff in (0.0, 1.5):
            r_c = 2.0 * h0
            got, sib = c.atom_forces_resident(origin, h0, xyz, q, v, r_c, cutoff), c2.atom_forces(xyz, q, v2, r_c, cutoff)
            for k in KEYS:
                assert got[k].shape == sib[k].shape and same_bits(got[k], sib[k]), (name, geometry, n, cutoff, k)
            if n == 40:
                assert np.isfinite(got["phi"]).all() and np.abs(got["phi"]).max() > 0 and np.abs(got["field"]).max() > 0
                assert (got["field"][33:36] == 0).all()    # far outside: no octant stays in the lattice
    v.free()
    v2.free()


def test_forces_on_zero_cells(ctx):
    fc = mtr.empty(3)
    build(ctx, fc)
    ctx.build_point_locator_resident(**kw(fc))
    assert len(ctx.get_point_locator()) == 0
    xyz, q = erc.atom_set(erc.forest("lattice-2"), 0.0, 1.0, 40)
    out = ctx.atom_forces_resident(0.0, 1.0, xyz, q, None, 0.5, 0.0, n_u=0)
    assert (out["phi"] == 0).all() and (out["field"] == 0).all() and same_bits(out["force"], out["force_short"]) and np.abs(out["e_short"]).max() > 0
    e = ctx.electrostatic_energy_resident(0.0, 1.0, xyz, q, None, 0.5, 0.0, n_u=0)
    short, fe, self_e = erc.energy_sums(q, out["phi"], out["e_short"], 0.5)
    assert same_bits(e.short, short) and e.fe_long == 0.0 and same_bits(e.self_energy, self_e)


# ------------------------------------------------------------------------------------------------ 3. the energy

@pytest.mark.parametrize("name", sorted(erc.FORESTS))
def test_energy_is_the_ascending_sum_of_the_sibling_s_values(two, name):
    c, c2 = two
    fc = erc.forest(name)
    t = build(c, fc)
    c.build_point_locator_resident(**kw(fc))
    u = noisy(t.n_dofs, 13)
    v, v2 = c.vector(t.n_dofs, u), c2.vector(t.n_dofs, u)
    for geometry, (origin, h0) in sorted(erc.GEOMETRY.items()):
        c2.set_point_locator(fc.n0, [origin] * 3, h0, erc.node_array(fc), t.cell_dofs)
        for n in (0, 1, 40):
            xyz, q = erc.atom_set(fc, origin, h0, n)
            for cutoff in (0.0, 1.5):
                r_c = 2.0 * h0
                sib = c2.atom_forces(xyz, q, v2, r_c, cutoff)
                want = erc.energy_sums(q, sib["phi"], sib["e_short"], r_c)
                first = None
                for force_block, max_blocks in ((64, 0), (128, 1), (256, 3)):
                    c.set_option("force_block", force_block)
                    c.set_option("assemble_max_blocks", max_blocks)
                    e = c.electrostatic_energy_resident(origin, h0, xyz, q, v, r_c, cutoff)
                    got = (e.short, e.fe_long, e.self_energy)
                    for k in range(3):
                        assert same_bits(got[k], want[k]), (name, geometry, n, cutoff, force_block, k, got[k], want[k])
                    first = first or got
                    assert first == got
                c.set_option("force_block", 64)
                c.set_option("assemble_max_blocks", 0)
                if n == 0:
                    assert got == (0.0, 0.0, 0.0)
    v.free()
    v2.free()


@pytest.mark.parametrize("case_id", erc.ENERGY_PAIR_CASES)
def test_short_sum_within_the_derived_bound(ctx, case_id):
    """short against both references of tests/atoms_reference.py, the bound B of tests/energy_resident_cases.py from each
    reference's own values; several tiles of the sum kernel where n > 256"""
    R = erc.pair_case(case_id)
    fc = erc.forest("lattice-2")
    t = build(ctx, fc)
    ctx.build_point_locator_resident(**kw(fc))
    v = ctx.vector(t.n_dofs, np.zeros(t.n_dofs))
    e = ctx.electrostatic_energy_resident(-2.0, 1.0, R.x, R.q, v, R.r_c, R.cutoff)
    v.free()
    for tier in ("mp", "np"):
        ref = getattr(R, tier)
        exact, bound = float(np.sum(ref["e"])) if tier == "np" else float(erc.ar.mp.fsum(erc.ar.mpf(x) for x in ref["e"])), erc.short_bound(ref)
        print(f"{case_id} {tier}: short {e.short!r} reference {exact!r} error {abs(e.short - exact):.3e} bound {bound:.3e}")
        assert abs(e.short - exact) <= bound, (case_id, tier, e.short, exact, bound)
    assert e.fe_long == 0.0 and same_bits(e.self_energy, erc.energy_sums(R.q, np.zeros(len(R.q)), np.zeros(len(R.q)), R.r_c)[2])


# ------------------------------------------------------------------------------------------------ 4. lifetime

def test_a_new_build_and_reset_drop_the_locator(ctx):
    A = capi()
    fc = erc.forest("deep")
    for keep in (1, 0):
        t = build(ctx, fc)
        ctx.build_point_locator_resident(**kw(fc))
        node = ctx.get_point_locator()
        ctx.set_option("reset_keeps_mesh_tables", keep)
        assert ctx.L.gmg_reset(ctx.h, C.c_int(2)) == A.OK
        ctx.set_option("reset_keeps_mesh_tables", 0)
        if keep:
            assert holds(ctx) and np.array_equal(ctx.get_point_locator(), node)
            v = ctx.vector(t.n_dofs, noisy(t.n_dofs))
            xyz, q = erc.atom_set(fc, -0.5, 0.25, 40)
            assert np.abs(ctx.atom_forces_resident(-0.5, 0.25, xyz, q, v, 0.5)["phi"]).max() > 0
            v.free()
        else:
            assert refused(A.ERR_INVALID, ctx.get_point_locator, "no mesh tables")
    build(ctx, fc)
    ctx.build_point_locator_resident(**kw(fc))
    assert holds(ctx)
    build(ctx, fc)   # a new build drops it
    assert not holds(ctx)
    # the locator of gmg_set_point_locator is another one: neither form sees the other's
    t = build(ctx, fc)
    v = ctx.vector(t.n_dofs, noisy(t.n_dofs))
    xyz, q = erc.atom_set(fc, -0.5, 0.25, 1)
    ctx.set_point_locator(fc.n0, [-0.5] * 3, 0.25, erc.node_array(fc), t.cell_dofs)
    assert refused(A.ERR_INVALID, lambda: ctx.atom_forces_resident(-0.5, 0.25, xyz, q, v, 0.5), "no point locator")
    assert ctx.L.gmg_reset(ctx.h, C.c_int(1)) == A.OK
    t = build(ctx, fc)
    ctx.build_point_locator_resident(**kw(fc))
    assert refused(A.ERR_INVALID, lambda: ctx.atom_forces(xyz, q, v, 0.5), "gmg_set_point_locator")
    v.free()


def test_unsupported_on_a_communicator_and_for_2d_tables():
    A = capi()
    c = A.Context(1)
    fc = erc.forest("lattice-2")
    xyz, q = erc.atom_set(fc, 0.0, 1.0, 1)
    v = c.vector(27, noisy(27))
    calls = (lambda: c.build_point_locator_resident(**kw(fc)), c.get_point_locator, lambda: c.atom_forces_resident(0.0, 1.0, xyz, q, v, 0.5),
             lambda: c.electrostatic_energy_resident(0.0, 1.0, xyz, q, v, 0.5))
    flat = rc.hand("staircase-2d").fc
    build(c, flat)
    for call in calls[1:] + (lambda: c.build_point_locator_resident(**kw(flat)),):
        assert refused(A.ERR_UNSUPPORTED, call, "3D")
    c.comm_init(0, 1, A.Context.unique_id())
    for call in calls:
        assert refused(A.ERR_UNSUPPORTED, call, "communicator")
    v.free()
    c.close()


def test_no_leak_over_six_rounds():
    """as tests/test_gpu_lifecycle.py: build, locator, forces, energy, reset, six times in one context; the free device memory
    after the last round equals that after the first"""
    import torch

    fc = erc.forest("wide")
    xyz, q = erc.atom_set(fc, -0.5, 0.25, 40)
    c = capi().Context(1)
    free = []
    for _ in range(6):
        t = build(c, fc)
        assert c.build_point_locator_resident(**kw(fc)).n_nodes == len(fc.cell_first_child)
        v = c.vector(t.n_dofs, noisy(t.n_dofs))
        assert np.abs(c.atom_forces_resident(-0.5, 0.25, xyz, q, v, 0.5, 1.5)["force"]).max() > 0
        assert c.electrostatic_energy_resident(-0.5, 0.25, xyz, q, v, 0.5, 1.5).self_energy > 0
        v.free()
        assert c.L.gmg_reset(c.h, C.c_int(1)) == capi().OK
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    c.close()
    print("free device memory after each round, relative to the first:", [f - free[0] for f in free])
    assert free[-1] == free[0], free


# ------------------------------------------------------------------------------------------------ 5. whole runs of the driver

ALL_KEYS = dict(mesh_tables_on_device=True, system_matrix_on_device=True, level_matrices_on_device=True, rhs_from_cell_tables=True,
                operators_from_resident_tables=True, estimator_on_device=True, analytical_on_device=True, refinement_on_device=True, transfer_on_device=True,
                densities_from_resident_tables=True, estimator_from_resident_tables=True, compute_forces=True)
ENERGY_LINES = ("Short-ranged energy contribution", "FE solution long-ranged energy contribution", "Self energy contribution",
                "Total electrostatic energy with split", "Absolute Error between both energies", "Relative Error in total electrostatic energy")
#  the lines whose values carry the short-range sum (within the bound, not by bits), and the one only a run with the key off prints
LOOSE = (ENERGY_LINES[0],) + ENERGY_LINES[3:]


def gas300(right):
    """300 atoms, the least the energy's large-system gate lets through: uniform in the box, no two closer than 0.25, neutral"""
    rng = np.random.default_rng(300)
    pts = []
    while len(pts) < 300:
        p = rng.uniform(0.2, right - 0.2, 3)
        if all(np.linalg.norm(p - o) >= 0.25 for o in pts):
            pts.append(p)
    return np.tile([1.0, -1.0], 150), np.array(pts)


def golden_problem(atoms, right, cycles, vacuum, key, **more):
    S = pkg().step50
    args = dict(ALL_KEYS)
    args.update(more)
    p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=vacuum, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=cycles, r_c=0.5,
                             cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR", refinement_estimator="Kelly",
                             energy_forces_from_resident_tables=key, **args))
    if isinstance(atoms, str):
        p.read_lammps(atoms)
    else:
        p.set_atoms(*atoms)
    return p


def norm_log(text):
    return [l for l in text.splitlines() if not any(k in l for k in LOOSE) and "seconds" not in l and " ms" not in l]


def driver_runs(make, cycles, short_cutoff):
    runs = {}
    for key in (False, True):
        p = make(key)
        out = []
        for cycle in range(cycles):
            rep = p.run_cycle(cycle, on_device=True)
            assert p.energy_forces_resident() == key and p.operators_resident() and p.mesh_tables_on_device(), (key, cycle)
            out.append((rep, p.atom_forces(parts=True), p.vector("solution"), p.marks()))
        log = p.log()
        assert "Energy and forces from resident tables" not in log, log   # no fallback line
        for line in ENERGY_LINES:
            assert log.count(line) == cycles, (key, line)
        builds = p.dof_map_builds()
        assert builds == 0 if key else builds >= 1, (key, builds)   # with the key off the energy is the first use of the host's maps
        q, xyz = p.atoms()
        runs[key] = (out, norm_log(log), np.asarray(q, float), np.asarray(xyz, float).reshape(-1, 3))
        p.close()
    assert runs[False][1] == runs[True][1]
    q, xyz = runs[True][2], runs[True][3]
    ref = erc.ar.pair_sums_numpy(xyz, q, 0.5, short_cutoff)
    B, exact = erc.short_bound(ref), float(ref["e"].sum())
    B_host = erc.host_short_bound(xyz, q, 0.5, short_cutoff, ref)
    for cycle, (a, b) in enumerate(zip(runs[False][0], runs[True][0])):
        for k in ("energy_fe_long", "energy_self", "force_max", "cg_iterations", "refine_threshold", "dofs", "active_cells"):
            assert repr(a[0][k]) == repr(b[0][k]), (cycle, k, a[0][k], b[0][k])
        assert repr(list(a[0]["force_net"])) == repr(list(b[0]["force_net"])), cycle
        for x, y in zip(a[1], b[1]):     # phi, field, force, force_short, e_short of every atom
            assert same_bits(x, y), cycle
        assert same_bits(a[2], b[2]) and np.array_equal(a[3], b[3]), cycle
        print(f"cycle {cycle}: energy_short host {a[0]['energy_short']!r} device {b[0]['energy_short']!r} numpy {exact!r}; bound device {B:.3e} host {B_host:.3e}")
        assert abs(b[0]["energy_short"] - exact) <= B and abs(a[0]["energy_short"] - b[0]["energy_short"]) <= B + B_host, cycle
        assert repr(b[0]["energy_total"]) == repr(b[0]["energy_short"] + b[0]["energy_fe_long"] - b[0]["energy_self"])
    return runs


CASES = {"8-atoms-3-cycles": (erc.GOLDEN_8, 1.0, 3, 10, {}, 0.0),
         "216-atoms-2-cycles": (erc.GOLDEN_216, 3.0, 2, 2, dict(energy_for_large_systems=True, short_range_cutoff=2.5), 2.5),
         "300-atoms-2-cycles": ("gas300", 3.0, 2, 2, dict(energy_for_large_systems=True, short_range_cutoff=2.5), 2.5)}   # past the 300-atom gate


@pytest.mark.parametrize("case", sorted(CASES))
def test_driver_runs_with_the_key_off_and_on(case, monkeypatch):
    monkeypatch.setenv("STEP50_CHECK_RESIDENT", "1")
    atoms, right, cycles, vacuum, more, short_cutoff = CASES[case]
    if atoms == "gas300":
        atoms = gas300(right)
    runs = driver_runs(lambda key: golden_problem(atoms, right, cycles, vacuum, key, **more), cycles, short_cutoff)
    last = runs[True][0][-1]
    assert last[0]["cg_iterations"] >= 1 and len(last[0]["dofs_by_level"]) >= 2 and np.abs(last[1][2]).max() > 0
    if case.startswith("300"):
        assert "not evaluated: all pairs of 300 atoms" in "\n".join(runs[True][1])


@pytest.mark.parametrize("missing,why", [("operators_from_resident_tables", "Operators from resident tables did not take effect"),
                                         ("rhs_from_cell_tables", None)])
def test_a_missing_prerequisite_keeps_the_host_path(missing, why):
    """one line says why, once over two cycles, and the run is the one without the key.  Without "RHS from cell tables" the
    operators do not become resident either, which is the reason given first; "the solution is not on the device" is the line
    of a solution set from outside (below)."""
    p, q = (golden_problem(erc.GOLDEN_8, 1.0, 2, 2, key, **{missing: False}) for key in (True, False))
    for cycle in range(2):
        r1, r0 = p.run_cycle(cycle, on_device=True), q.run_cycle(cycle, on_device=True)
        assert not p.energy_forces_resident()
        for k in ("energy_short", "energy_fe_long", "energy_self", "energy_total", "force_max", "cg_iterations"):
            assert repr(r1[k]) == repr(r0[k]), (cycle, k)
        for x, y in zip(p.atom_forces(parts=True), q.atom_forces(parts=True)):
            assert same_bits(x, y)
    said = [l for l in p.log().splitlines() if "Energy and forces from resident tables" in l]
    assert len(said) == 1 and "Energy and forces from resident tables" not in q.log(), said
    assert said[0] == LINE.format(why or "Operators from resident tables did not take effect") or (why is None and said[0] == LINE.format("the solution is not on the device"))
    p.close()
    q.close()


def test_a_solution_set_from_outside_is_not_on_the_device():
    p = golden_problem(erc.GOLDEN_8, 1.0, 1, 2, True)
    p.run_cycle(0, on_device=True)
    assert p.energy_forces_resident()
    p.finish_cycle_with(p.vector("solution"))     # the host's copy takes the place of the device's
    assert not p.energy_forces_resident() and p.log().count(LINE.format("the solution is not on the device")) == 1
    p.close()


def test_a_distributed_run_and_a_problem_without_atoms_keep_the_host_path():
    p = golden_problem(erc.GOLDEN_8, 1.0, 1, 2, True)
    p.set_communicator(0, 1, capi().Context.unique_id())
    p.run_cycle(0, on_device=True)
    assert not p.energy_forces_resident() and p.log().count(LINE.format("the run is distributed")) == 1
    p.close()
    keys = {k: v for k, v in ALL_KEYS.items() if k not in ("densities_from_resident_tables", "compute_forces")}
    s = step16_problem(3, 2, 2, energy_forces_from_resident_tables=True, **keys)
    for cycle in range(2):
        s.run_cycle(cycle, on_device=True)
    assert s.operators_resident() and not s.energy_forces_resident()
    assert s.log().count(LINE.format("not a 3D problem with LAMMPS input")) == 1
    s.close()
