"""gmg_assemble_rhs and gmg_distribute_constraints on the MI355X (csrc/gmg_rhs_cells.hpp) through the C ABI:
against the restatement of tests/rhs_cells_reference.py and the host driver's vectors on the meshes of
tests/test_rhs_cells_cpu.py, with device-resident densities, with synthetic tables, on hand-built inputs; the refusals; and whole
runs of the driver with "RHS from cell tables" off and on.  The definition fixes every operand order: all comparisons are of bits."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import rhs_cells_reference as rcr
import test_rhs_cells_cpu as cpu
from conftest import rel_close
from gpu_util import capi, pkg
from test_coef_matrix_cpu import step16_problem

pytestmark = pytest.mark.gpu

K2D = np.array([[4, -1, -1, -2], [-1, 4, -2, -1], [-1, -2, 4, -1], [-2, -1, -1, 4]], dtype=np.float64) / 6.0   # the Q1 Laplacian of a square


@pytest.fixture()
def ctx():
    c = capi().Context(1)
    yield c
    c.close()


def device_rhs(c, inp, fill=7.0, **kw):
    """the vector gmg_assemble_rhs leaves in a device vector that held `fill` everywhere"""
    v = c.vector(max(inp.n_dofs, 1), np.full(max(inp.n_dofs, 1), fill))
    try:
        c.assemble_rhs(inp, v, **kw)
        return v.download()[:inp.n_dofs]
    finally:
        v.free()


def changed(inp, **kw):
    d = dict(vars(inp))
    d.update(kw)
    return SimpleNamespace(**d)


def with_entry(a, i, v):
    a = np.array(a)
    a.reshape(-1)[i] = v
    return a


# ------------------------------------------------------------------------------------------------ 1. the meshes of the CPU tests

@pytest.mark.parametrize("name", cpu.CASES)
def test_device_equals_reference_and_host(name):
    x = cpu.case(name)
    ref = cpu.reference(name)
    assert rcr.same_bits(ref, x.rhs)
    for max_blocks in (0, 1, 3):   # by size; one workgroup; three (every grid-stride loop iterates)
        c = capi().Context(1)
        c.set_option("assemble_max_blocks", max_blocks)
        got = device_rhs(c, x.inp)
        c.close()
        assert rcr.same_bits(got, ref), (name, max_blocks, int(np.sum(got != ref)))


def test_device_resident_densities_equal_the_same_values_as_source(ctx):
    """source = NULL takes what gmg_charge_density(dens = NULL) left on the device: the bits of the same densities passed in"""
    x = cpu.case("A3")
    inp = x.inp
    n_cells, nq = inp.source.shape
    rng = np.random.default_rng(5)
    lo = rng.uniform(0.0, 1.0, (n_cells, 3))
    h = np.full(n_cells, 0.25)
    atoms, q = rng.uniform(0.0, 1.25, (5, 3)), rng.uniform(-1.0, 1.0, 5)
    qp = rng.uniform(0.0, 1.0, (nq, 3))
    with pytest.raises(capi().GMGError) as e:   # nothing on the device yet
        device_rhs(ctx, inp, source=None)
    assert e.value.code == capi().ERR_INVALID
    assert ctx.charge_density(lo, h, np.floor(lo), 1.0, atoms, q, 0.5, 10.0, False, qp, dens=None) is None
    dens = ctx.get_charge_density(n_cells, nq)
    assert np.count_nonzero(dens) > dens.size // 2
    resident = device_rhs(ctx, inp, source=None)
    passed = device_rhs(ctx, inp, source=dens)
    assert rcr.same_bits(resident, passed) and rcr.same_bits(resident, rcr.assemble(inp, dens))
    with pytest.raises(capi().GMGError) as e:   # densities of another shape
        device_rhs(ctx, changed(inp, nq=1, shape=inp.shape[:1], weight=inp.weight[:1]), source=None)
    assert e.value.code == capi().ERR_INVALID


def synthetic(inp, nq, seed):
    """the cell tables of inp with seeded random quadrature tables, source and inhomogeneities (on every line: hanging-node
    lines inherit values in the driver, too), and a cell matrix without symmetry"""
    rng = np.random.default_rng(seed)
    nv = 1 << inp.dim
    n_lines = len(inp.line_ptr) - 1
    li = rng.standard_normal(n_lines)
    li[rng.random(n_lines) < 0.3] = 0.0
    return changed(inp, nq=nq, shape=rng.standard_normal((nq, nv)), weight=rng.uniform(0.1, 1.0, nq), jxw_of_level=rng.uniform(0.01, 1.0, 16),
                   source=rng.standard_normal((len(inp.cell_level), nq)), line_inhomogeneity=li, K_of_level=rng.standard_normal((16, nv, nv)))


@pytest.mark.parametrize("nq", (1, 8, 27))
@pytest.mark.parametrize("name", ("A3", "B3", "S2-c1"))
def test_synthetic_tables(ctx, name, nq):
    inp = synthetic(cpu.case(name).inp, nq, 100 * nq + len(name))
    assert rcr.same_bits(device_rhs(ctx, inp), rcr.assemble(inp)), (name, nq)


# ------------------------------------------------------------------------------------------------ 2. hand-built 2D inputs

def tables_2d(cells, levels, n_dofs, cons, line_ptr, master, weight, inhom, seed, nq=4):
    rng = np.random.default_rng(seed)
    return SimpleNamespace(dim=2, n_dofs=n_dofs, cell_dofs=np.array(cells, dtype=np.int32).reshape(-1, 4), cell_level=np.array(levels, dtype=np.uint8),
                           K_of_level=np.tile(K2D, (16, 1, 1)), constraint_of_dof=np.array(cons, dtype=np.int32),
                           line_ptr=np.array(line_ptr, dtype=np.int64), line_master=np.array(master, dtype=np.int32),
                           line_weight=np.array(weight, dtype=np.float64), line_inhomogeneity=np.array(inhom, dtype=np.float64), nq=nq,
                           shape=rng.uniform(0.0, 1.0, (nq, 4)), weight=rng.uniform(0.1, 1.0, nq), jxw_of_level=0.25 ** np.arange(16),
                           source=rng.standard_normal((len(levels), nq)))


def quadrant_mesh(dirichlet_value):
    """3 x 3 cells whose bottom middle cell is cut in four (the mesh of tests/test_gpu_system_matrix.py, rebuilt here): 12 cells,
    21 vertices, three hanging nodes -- two with one interior master (weight 0.5: the other master is on the boundary, whose
    value the resolved line carries as its inhomogeneity), one with two.  Every boundary vertex is on a Dirichlet line of value
    dirichlet_value(x, y)."""
    pts = {}

    def dof(x, y):
        return pts.setdefault((x, y), len(pts))

    cells, levels = [], []
    for y in (0, 2, 4):
        for x in (0, 2, 4):
            if (x, y) != (2, 0):
                cells.append([dof(x, y), dof(x + 2, y), dof(x, y + 2), dof(x + 2, y + 2)])
                levels.append(1)
    for x, y in ((2, 0), (3, 0), (2, 1), (3, 1)):
        cells.append([dof(x, y), dof(x + 1, y), dof(x, y + 1), dof(x + 1, y + 1)])
        levels.append(2)
    cons = -np.ones(len(pts), dtype=np.int32)
    line_ptr, master, weight, inhom = [0], [], [], []

    def add_line(d, ent, g):
        cons[d] = len(line_ptr) - 1
        for m, w in ent:
            master.append(m)
            weight.append(w)
        line_ptr.append(len(master))
        inhom.append(g)

    for (x, y), d in sorted(pts.items(), key=lambda t: t[1]):
        if x in (0, 6) or y in (0, 6):
            add_line(d, [], dirichlet_value(x, y))
    add_line(pts[(2, 1)], [(pts[(2, 2)], 0.5)], 0.5 * dirichlet_value(2, 0))
    add_line(pts[(4, 1)], [(pts[(4, 2)], 0.5)], 0.5 * dirichlet_value(4, 0))
    add_line(pts[(3, 2)], [(pts[(2, 2)], 0.5), (pts[(4, 2)], 0.5)], 0.0)
    return tables_2d(cells, levels, len(pts), cons, line_ptr, master, weight, inhom, seed=21)


def fan(n_cells):
    """n_cells cells that all hold DoF 0 and three DoFs of their own; in every third cell the second vertex hangs on DoF 0 (and on
    the cell's fourth vertex), in every fifth the third vertex is on a Dirichlet line with a value: DoF 0 collects from more than
    n_cells slots, through its own vertex and as a master"""
    cells = [[0, 3 * c + 1, 3 * c + 2, 3 * c + 3] for c in range(n_cells)]
    cons = -np.ones(3 * n_cells + 1, dtype=np.int32)
    line_ptr, master, weight, inhom = [0], [], [], []
    for c in range(n_cells):
        if c % 3 == 0:
            cons[3 * c + 1] = len(inhom)
            master += [0, 3 * c + 3]
            weight += [0.5, 0.25]
            inhom.append(0.0)
            line_ptr.append(len(master))
        if c % 5 == 0:
            cons[3 * c + 2] = len(inhom)
            inhom.append(1.0 + 0.125 * c)
            line_ptr.append(len(master))
    return tables_2d(cells, [c % 3 for c in range(n_cells)], 3 * n_cells + 1, cons, line_ptr, master, weight, inhom, seed=100)


def test_quadrant_mesh_with_hanging_nodes(ctx):
    for value in (lambda x, y: 0.0, lambda x, y: 1.0 + 0.25 * x + 0.5 * y):   # homogeneous; every Dirichlet value nonzero
        inp = quadrant_mesh(value)
        assert inp.cell_dofs.shape == (12, 4) and np.sum(np.diff(inp.line_ptr) > 0) == 3
        ref = rcr.assemble(inp)
        assert rcr.same_bits(device_rhs(ctx, inp), ref)
        assert np.all(ref[inp.constraint_of_dof >= 0] == 0.0) and np.any(ref != 0.0)   # constrained DoFs receive nothing
    assert np.all(inp.line_inhomogeneity[np.diff(inp.line_ptr) == 0] != 0.0)
    # without inhomogeneities the cell matrix is not needed
    hom = quadrant_mesh(lambda x, y: 0.0)
    assert rcr.same_bits(device_rhs(ctx, hom, K_of_level=None), rcr.assemble(hom))


def test_fan_of_100_cells(ctx):
    """the slot walk of DoF 0 is 100 slots of its own vertex and 34 through hanging nodes"""
    inp = fan(100)
    ref = rcr.assemble(inp)
    for max_blocks in (0, 1):
        ctx.set_option("assemble_max_blocks", max_blocks)
        assert rcr.same_bits(device_rhs(ctx, inp), ref)
    assert ref[0] != 0.0 and rcr.features(inp)[1] == 20


def test_all_dirichlet_cells_give_positive_zero(ctx):
    """two cells whose vertices are all on Dirichlet lines with values: F is formed and passed on to nobody; two DoFs belong to
    no cell at all"""
    cons = np.array([0, 1, 2, 3, 4, 5, -1, -1], dtype=np.int32)
    inp = tables_2d([[0, 1, 2, 3], [1, 4, 3, 5]], [0, 1], 8, cons, [0] * 7, [], [], [1.0, -2.0, 3.0, 0.5, 0.25, -1.0], seed=3)
    got = device_rhs(ctx, inp, fill=-3.0)
    assert np.array_equal(got.view(np.uint64), np.zeros(8, dtype=np.uint64))
    assert np.any(rcr.slot_values(inp) != 0.0)


def test_zero_cells(ctx):
    inp = SimpleNamespace(dim=3, n_dofs=5, cell_dofs=np.zeros((0, 8), dtype=np.int32), cell_level=np.zeros(0, dtype=np.uint8), K_of_level=None,
                          constraint_of_dof=-np.ones(5, dtype=np.int32), line_ptr=None, line_master=None, line_weight=None, line_inhomogeneity=None,
                          nq=8, shape=np.ones((8, 8)), weight=np.ones(8), jxw_of_level=np.ones(16), source=None)
    got = device_rhs(ctx, inp, fill=-3.0)
    assert np.array_equal(got.view(np.uint64), np.zeros(5, dtype=np.uint64))


# ------------------------------------------------------------------------------------------------ 3. refusals

def test_invalid_arguments_are_refused_and_rhs_is_untouched(ctx):
    A = capi()
    good = quadrant_mesh(lambda x, y: 1.0 + x)
    n_lines = len(good.line_ptr) - 1
    lp_dec = with_entry(good.line_ptr, n_lines - 1, good.line_ptr[-1] + 1)
    bad = {
        "dim": changed(good, dim=4),
        "dof below": changed(good, cell_dofs=with_entry(good.cell_dofs, 5, -1)),
        "dof above": changed(good, cell_dofs=with_entry(good.cell_dofs, 5, good.n_dofs)),
        "master below": changed(good, line_master=with_entry(good.line_master, 0, -1)),
        "master above": changed(good, line_master=with_entry(good.line_master, 0, good.n_dofs)),
        "line index above": changed(good, constraint_of_dof=with_entry(good.constraint_of_dof, 0, n_lines)),
        "line index below": changed(good, constraint_of_dof=with_entry(good.constraint_of_dof, 0, -2)),
        "line_ptr start": changed(good, line_ptr=with_entry(good.line_ptr, 0, -1)),
        "line_ptr decreases": changed(good, line_ptr=lp_dec),
        "level": changed(good, cell_level=with_entry(good.cell_level, 0, 16)),
        "nq 0": changed(good, nq=0),
        "nq 513": changed(good, nq=513),
        "null constraint_of_dof": changed(good, constraint_of_dof=np.zeros(0, dtype=np.int32)),
        "null cell_dofs": changed(good, cell_dofs=np.zeros(0, dtype=np.int32)),
        "null shape": changed(good, shape=None),
        "null weight": changed(good, weight=None),
        "null jxw": changed(good, jxw_of_level=None),
        "null inhomogeneity": changed(good, line_inhomogeneity=None),
        "null line_weight": changed(good, line_weight=None),
        "no densities": changed(good, source=None),
        "K null with a value": changed(good, K_of_level=None),
    }
    v = ctx.vector(good.n_dofs, np.full(good.n_dofs, 7.0))
    for what, inp in bad.items():
        with pytest.raises(A.GMGError) as e:
            ctx.assemble_rhs(inp, v)
        assert e.value.code == A.ERR_INVALID and "gmg_assemble_rhs" in str(e.value), what
        assert np.all(v.download() == 7.0), what
    with pytest.raises(A.GMGError) as e:   # a NULL rhs of nonzero length
        ctx.assemble_rhs(good, None)
    assert e.value.code == A.ERR_INVALID
    ctx.assemble_rhs(good, v)   # the context survives
    assert rcr.same_bits(v.download(), rcr.assemble(good))
    v.free()


def test_unsupported_on_a_communicator():
    A = capi()
    c = A.Context(1)
    c.comm_init(0, 1, A.Context.unique_id())
    good = quadrant_mesh(lambda x, y: 1.0)
    v = c.vector(good.n_dofs, np.full(good.n_dofs, 7.0))
    with pytest.raises(A.GMGError) as e:
        c.assemble_rhs(good, v)
    assert e.value.code == A.ERR_UNSUPPORTED and "not on a communicator" in str(e.value)
    assert np.all(v.download() == 7.0)
    c.close()


# ------------------------------------------------------------------------------------------------ 4. gmg_distribute_constraints

def distribute(c, inp, u):
    v = c.vector(len(u), u)
    try:
        c.distribute_constraints(v, inp.constraint_of_dof, inp.line_ptr, inp.line_master, inp.line_weight, inp.line_inhomogeneity)
    finally:
        out = v.download()
        v.free()
    return out


@pytest.mark.parametrize("name", ("A3", "B3"))
def test_distribute_equals_the_host(ctx, name):
    x = cpu.case(name)
    for max_blocks in (0, 1, 3):
        ctx.set_option("assemble_max_blocks", max_blocks)
        got = distribute(ctx, x.inp, x.x)
        assert rcr.same_bits(got, x.sol) and rcr.same_bits(got, rcr.distribute(x.inp, x.x)), (name, max_blocks)
    assert np.any(x.sol != x.x)


def test_distribute_refuses_a_constrained_master(ctx):
    A = capi()
    good = quadrant_mesh(lambda x, y: 1.0 + x)
    u = np.cos(np.arange(good.n_dofs) * 0.7)
    assert rcr.same_bits(distribute(ctx, good, u), rcr.distribute(good, u))
    dirichlet = int(np.flatnonzero(good.constraint_of_dof >= 0)[0])
    bad = {"constrained master": changed(good, line_master=with_entry(good.line_master, 0, dirichlet)),
           "master above": changed(good, line_master=with_entry(good.line_master, 0, good.n_dofs)),
           "line index": changed(good, constraint_of_dof=with_entry(good.constraint_of_dof, 0, len(good.line_ptr) - 1)),
           "line_ptr decreases": changed(good, line_ptr=with_entry(good.line_ptr, len(good.line_ptr) - 2, good.line_ptr[-1] + 1))}
    for what, inp in bad.items():
        v = ctx.vector(len(u), u)
        with pytest.raises(A.GMGError) as e:
            ctx.distribute_constraints(v, inp.constraint_of_dof, inp.line_ptr, inp.line_master, inp.line_weight, inp.line_inhomogeneity)
        assert e.value.code == A.ERR_INVALID and "gmg_distribute_constraints" in str(e.value), what
        assert rcr.same_bits(v.download(), u), what
        v.free()


# ------------------------------------------------------------------------------------------------ 5. whole runs of the driver

SKIP_KEYS = ("solve_seconds", "build_matrices_ms")   # times
# energy_norm_error is an OpenMP reduction over the cells in the order the threads finish (postprocess_error_in_energy_norm): its
# last bits differ between two runs of one configuration.  A sum of n non-negative terms in any order, then a square root: two
# such values differ by at most (n + 2) 2^-53 relative, each from the exact one.
UNORDERED_SUMS = ("energy_norm_error",)


def driver_runs(make, cycles, after=None):
    """the same run with the key off and on: per cycle the report, the marks, the right-hand side, the solution (and what
    `after` takes from the problem).  Everything but the times must be equal."""
    runs = {}
    for key in (False, True):
        p = make(key)
        out = []
        for cycle in range(cycles):
            rep = p.run_cycle(cycle, on_device=True)
            assert p.rhs_from_cell_tables() == key, cycle
            out.append((rep, p.refine_flags(), p.vector("rhs"), p.vector("solution"), after(p) if after else None))
        assert "RHS from cell tables" not in p.log(), p.log()   # no fallback line
        runs[key] = out
        p.close()
    for cycle, (a, b) in enumerate(zip(runs[False], runs[True])):
        for k in a[0]:
            if k in UNORDERED_SUMS:
                assert abs(a[0][k] - b[0][k]) <= 2 * (a[0]["active_cells"] + 2) * 2.0 ** -53 * abs(a[0][k]), (cycle, k, a[0][k], b[0][k])
            elif k not in SKIP_KEYS:
                assert repr(a[0][k]) == repr(b[0][k]), (cycle, k, a[0][k], b[0][k])
        assert np.array_equal(a[1], b[1]), cycle
        assert rcr.same_bits(a[2], b[2]) and rcr.same_bits(a[3], b[3]), cycle
    return runs


def golden_make(golden_dir, name, right, cycles, smoother, **more):
    S = pkg().step50

    def make(key):
        p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=cycles,
                                 r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother=smoother,
                                 refinement_estimator="Kelly", rhs_from_cell_tables=key, **more))
        p.read_lammps(os.path.join(golden_dir, name))
        return p

    return make


ALL_ON = dict(system_matrix_on_device=True, level_matrices_on_device=True, estimator_on_device=True)
GOLDEN_RUNS = [("atom_n1_8.data", 1.0, 3, "SSOR", {}), ("atom_n1_8.data", 1.0, 3, "Jacobi", {}), ("atom_n1_8.data", 1.0, 3, "SSOR", ALL_ON),
               ("atom_n3_216.data", 3.0, 2, "SSOR", {})]


@pytest.mark.parametrize("name,right,cycles,smoother,more", GOLDEN_RUNS, ids=[f"{m[0]}-{m[3]}{'-all' if m[4] else ''}" for m in GOLDEN_RUNS])
def test_adaptive_run_is_unchanged(golden_dir, name, right, cycles, smoother, more):
    """the golden configurations (10 vacuum cells, Kelly marking): equal iteration counts, printed norms, residuals, thresholds,
    energies, marks, and the bits of system_rhs and of the distributed solution"""
    runs = driver_runs(golden_make(golden_dir, name, right, cycles, smoother, **more), cycles)
    last = runs[True][-1][0]
    assert len(last["dofs_by_level"]) >= 2 and last["cg_iterations"] >= 1


def test_device_solution_feeds_forces_and_error_norm(golden_dir):
    """the vector gmg_distribute_constraints left on the device is what gmg_atom_forces and gmg_energy_norm_error take: the same
    bits as with a re-uploaded host solution"""
    def after(p):
        return p.atom_forces(on_device=True) + p.cell_errors(on_device=True, norm=True)

    runs = driver_runs(golden_make(golden_dir, "atom_n1_8.data", 1.0, 2, "SSOR", estimator_on_device=True), 2, after)
    for cycle, (a, b) in enumerate(zip(runs[False], runs[True])):
        for u, v in zip(a[4], b[4]):
            assert rcr.same_bits(np.asarray(u), np.asarray(v)), cycle


@pytest.mark.parametrize("dim,refine", ((2, 3), (3, 2)))
def test_step16_run_is_unchanged(dim, refine):
    runs = driver_runs(lambda key: step16_problem(dim, refine, 3, rhs_from_cell_tables=key), 3)
    assert len(runs[True][-1][0]["dofs_by_level"]) >= refine + 2


def test_fallbacks_say_why_once(golden_dir):
    """densities that are not on the device: the host pass stays, with one line"""
    p = golden_make(golden_dir, "atom_n1_8.data", 1.0, 2, "SSOR", rhs_on_device=False)(True)
    q = golden_make(golden_dir, "atom_n1_8.data", 1.0, 2, "SSOR", rhs_on_device=False)(False)
    for cycle in range(2):
        r1, r0 = p.run_cycle(cycle, on_device=True), q.run_cycle(cycle, on_device=True)
        assert not p.rhs_from_cell_tables() and rcr.same_bits(p.vector("rhs"), q.vector("rhs")) and r1["cg_iterations"] == r0["cg_iterations"]
    assert p.log().count("RHS from cell tables: not applicable (the charge densities are not on the device)") == 1
    p.close()
    q.close()


def test_distributed_run_keeps_the_host_pass(golden_dir):
    """a run on a communicator (one rank): one line says why, the right-hand side is the host pass's"""
    p = golden_make(golden_dir, "atom_n1_8.data", 1.0, 1, "SSOR")(True)
    q = golden_make(golden_dir, "atom_n1_8.data", 1.0, 1, "SSOR")(False)
    p.set_communicator(0, 1, capi().Context.unique_id())
    r1, r0 = p.run_cycle(0, on_device=True), q.run_cycle(0, on_device=True)
    assert not p.rhs_from_cell_tables() and rcr.same_bits(p.vector("rhs"), q.vector("rhs")) and rcr.same_bits(p.vector("solution"), q.vector("solution"))
    assert r1["cg_iterations"] == r0["cg_iterations"]
    assert p.log().count("RHS from cell tables: not applicable (the run is distributed)") == 1
    p.close()
    q.close()


def test_rc_variation_rhs_norms_with_the_key(golden, golden_dir):
    """the setup of the reference's tests_rhs_rc_variation (tests/test_host.py): its printed rhs norms to their 11 digits"""
    g = golden["tests_rhs_rc_variation/rc_variation.mpirun=1"]["runs"][0]["cycles"][0]
    S = pkg().step50
    p = S.Problem(S.prm_text(left=-2.5, right=2.5, mesh_size=0.3125, vacuum=0, problem="GaussianCharges", dim=3, bc="Homogeneous", cycles=1, r_c=0.5,
                             cutoff=3.0, rhs_optimization=False, quad_rhs=1, global_refinement=0, smoother="Jacobi", densities_on_device=True,
                             rhs_from_cell_tables=True))
    p.read_lammps(os.path.join(golden_dir, "atom_2.data"))
    rep = p.run_cycle(0, on_device=True)
    assert p.rhs_from_cell_tables() and "not applicable" not in p.log()
    b = p.vector("rhs")
    print("rhs norms:", rep["rhs_l2"], rep["rhs_linf"], "golden:", g["rhs_l2"], g["rhs_linf"])
    assert rel_close(float(np.sqrt(b @ b)), g["rhs_l2"], 11) and rel_close(float(np.abs(b).max()), g["rhs_linf"], 11)
    assert rel_close(rep["rhs_l2"], g["rhs_l2"], 11) and rel_close(rep["rhs_linf"], g["rhs_linf"], 11)
    p.close()


def test_no_leak_across_cycles_with_the_key():
    """as tests/test_gpu_lifecycle.py: six rounds of a two-cycle run with the key on (the solution vector stays on the device
    between the solve and the next cycle, and until close()); the free device memory after the last equals that after the first"""
    import torch

    S = pkg().step50
    free = []
    for _ in range(6):
        p = S.Problem(S.prm_text(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=2, r_c=0.5,
                                 cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR", short_range_cutoff=6,
                                 estimator_on_device=True, rhs_from_cell_tables=True))
        try:
            p.set_nacl_atoms(1)
            for cycle in range(2):
                assert p.run_cycle(cycle, on_device=True)["cg_iterations"] >= 1 and p.rhs_from_cell_tables()
                assert np.isfinite(p.atom_forces(on_device=True)[2]).all()
        finally:
            p.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    print("free device memory after each round, relative to the first:", [f - free[0] for f in free])
    assert free[-1] == free[0], free
