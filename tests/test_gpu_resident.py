"""gmg_close_constraints and the resident forms of the assemblies, the right-hand side and the distribution on the MI355X
(csrc/gmg_close.hpp), through the C ABI: the closed lines against the restatement of
tests/close_reference.py and the host's closed lines; every resident entry against its host-array sibling in a second context
fed the downloaded tables and the host-closed lines; the refusals; the device memory over six rounds; and whole runs of the
driver with "Operators from resident tables" off and on.  Every definition fixes the operand order: all comparisons are of bits."""
import ctypes as C
import os

import numpy as np
import pytest

import close_reference as cr
import mesh_tables_cases as mtc
import mesh_tables_reference as mtr
import resident_cases as rc
from gpu_util import capi, pkg
from test_close_cpu import CASES as CLOSE_CASES, dirichlet_values, same_lines
from test_coef_matrix_cpu import step16_problem

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    c = capi().Context(1)
    yield c
    c.close()


def build(c, fc):
    return c.build_mesh_tables(dim=fc.dim, n0=fc.n0, n_levels=fc.n_levels, level_ptr=fc.level_ptr, cell_coord=fc.cell_coord,
                               cell_first_child=fc.cell_first_child, level0_lexicographic=fc.level0_lexicographic)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def vbits(v):
    return v.download().view(np.uint64)


def same_arrays(got, ref):
    """every array of ref (lists or arrays) in got, floating-point ones by their bits"""
    for k, w in vars(ref).items():
        v = getattr(got, k)
        assert np.array_equal(bits(v), bits(w)) if "weight" in k or "inhom" in k else np.array_equal(np.asarray(v), np.asarray(w)), k
    return True


def refused(code, call, text=None):
    with pytest.raises(capi().GMGError) as e:
        call()
    assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)
    return True


# ------------------------------------------------------------------------------------------------ 1. gmg_close_constraints

@pytest.mark.parametrize("name", CLOSE_CASES)
def test_close_equals_reference_and_host(name):
    x = mtc.case(name)
    values = dirichlet_values(x)
    ref = cr.close_tables(x.ref, values.tolist())
    other = np.cos(np.arange(len(values), dtype=np.float64)) * 3.0   # other values, none of them 0
    ref_other = cr.close_tables(x.ref, other.tolist())
    for max_blocks in (0, 1, 3):   # by size; one workgroup; three (the grid-stride loop iterates)
        c = capi().Context(1)
        c.set_option("assemble_max_blocks", max_blocks)
        build(c, x.fc)
        before = c.get_mesh_tables()
        assert c.close_constraints(other) >= 0.0
        assert same_arrays(c.get_closed_constraints(), ref_other)
        assert c.close_constraints(values) >= 0.0   # the second call replaces the first
        got = c.get_closed_constraints()
        assert same_arrays(got, ref) and same_lines(got, x.sys, (name, max_blocks))
        assert (got.n_lines, got.n_entries) == (x.ref.n_lines, len(ref.line_master))
        assert same_arrays(c.get_mesh_tables(), before)   # the unclosed tables are what they were
        c.close_constraints(None)   # NULL: all +0.0
        assert same_arrays(c.get_closed_constraints(), cr.close_tables(x.ref))
        c.close()


def test_close_hand_built_forests(ctx):
    for fc in (mtr.quadrant_2d(), mtr.edge_only_3d(), mtr.single_cell(3), mtr.empty(2)):
        ref = mtr.build(fc)
        build(ctx, fc)
        values = 1.0 + np.arange(ref.n_lines - ref.n_hanging, dtype=np.float64) / 7.0
        ctx.close_constraints(values, n_values=len(values))
        assert same_arrays(ctx.get_closed_constraints(), cr.close_tables(ref, values.tolist()))
    assert ctx.get_closed_constraints().line_ptr.tolist() == [0]   # zero lines are valid


# ------------------------------------------------------------------------------------------------ 2. the entries against their siblings

def resident_context(x, L, coef=False):
    c = capi().Context(L)
    build(c, x.fc)
    c.close_constraints(x.sys.line_inhomogeneity[c.get_mesh_tables().n_hanging:])
    return c


def load(c, x, resident, coef):
    """the operators by the resident entries, or by their siblings from the downloaded tables and the host-closed lines"""
    s = x.sys
    if resident and coef:
        c.assemble_system_matrix_coef_resident(x.sysc.nq, x.sysc.cell_coef, x.sysc.G, x.sysc.qw, x.sysc.scale_of_level)
    elif resident:
        c.assemble_system_matrix_resident(s.K_of_level)
    elif coef:
        c.assemble_system_matrix_coef(s.dim, s.n_dofs, s.cell_dofs, s.cell_level, x.sysc.nq, x.sysc.cell_coef, x.sysc.G, x.sysc.qw, x.sysc.scale_of_level,
                                      s.constraint_of_dof, s.line_ptr, s.line_master, s.line_weight)
    else:
        c.assemble_system_matrix(s.dim, s.n_dofs, s.cell_dofs, s.cell_level, s.K_of_level, s.constraint_of_dof, s.line_ptr, s.line_master, s.line_weight)
    for l in range(len(x.levels)):
        load_level(c, x, l, resident, coef)
        c.set_copy_indices(l, x.h.copy_global[l], x.h.copy_level[l])
    for l, P in enumerate(x.h.prolongations):
        c.set_prolongation(l, P)


def load_level(c, x, l, resident, coef):
    lv = x.levels[l]
    if resident and coef:
        k = x.levc[l]
        c.assemble_level_matrix_coef_resident(l, k.nq, k.cell_coef, k.G, k.qw, k.scale)
    elif resident:
        c.assemble_level_matrix_resident(l, lv.K)
    elif coef:
        k = x.levc[l]
        c.assemble_level_matrix_coef(l, lv.dim, lv.n_dofs, lv.cell_dofs, k.nq, k.cell_coef, k.G, k.qw, k.scale, lv.dof_flags)
    else:
        c.assemble_level_matrix(l, lv.dim, lv.n_dofs, lv.cell_dofs, lv.K, lv.dof_flags)


SIBLINGS = [(n, False) for n in rc.CASES] + [(n, True) for n in rc.STEP16]


@pytest.mark.parametrize("name,coef", SIBLINGS, ids=[f"{n}{'-coef' if k else ''}" for n, k in SIBLINGS])
def test_operators_equal_the_siblings(name, coef):
    """downloads, norms, SpMV, one step of Jacobi and of SSOR in 1 and 3 blocks, one V-cycle: identical bits"""
    A = capi()
    x = rc.case(name)
    L = len(x.levels)
    a, b = resident_context(x, L), A.Context(L)
    # the tables the sibling is fed are the downloaded ones, and they are the host's
    t = a.get_mesh_tables()
    assert np.array_equal(t.cell_dofs.reshape(x.sys.cell_dofs.shape), x.sys.cell_dofs) and np.array_equal(t.constraint_of_dof, x.sys.constraint_of_dof)
    assert same_lines(a.get_closed_constraints(), x.sys, name)
    load(a, x, True, coef)
    load(b, x, False, coef)
    Sa, Sb = a.get_system_matrix(), b.get_system_matrix()
    assert np.array_equal(Sa.rowptr, Sb.rowptr) and np.array_equal(Sa.col, Sb.col) and np.array_equal(bits(Sa.val), bits(Sb.val))
    assert a.system_matrix_norms()[:2] == b.system_matrix_norms()[:2]
    for l in range(L):
        for which in (A.LEVEL_A, A.LEVEL_EDGE, A.LEVEL_EDGE_T):
            Ma, Mb = a.get_level_matrix(l, which), b.get_level_matrix(l, which)
            assert Ma.nnz == Mb.nnz and np.array_equal(Ma.rowptr, Mb.rowptr) and np.array_equal(Ma.col, Mb.col) and np.array_equal(bits(Ma.val), bits(Mb.val)), (l, which)
    rng = np.random.default_rng(L)

    def both(f):
        return np.array_equal(f(a), f(b))

    for which, n in [(A.SYSTEM, x.sys.n_dofs)] + [(l, lv.n_dofs) for l, lv in enumerate(x.levels)]:
        v = rng.standard_normal(n)

        def spmv(c):
            vx, vy = c.vector(n, v), c.vector(n)
            c.spmv(which, vy, vx)
            return vbits(vy)
        assert both(spmv), (name, "spmv", which)

    def smooth_all(what):
        for l in range(1, L):
            n = x.levels[l].n_dofs
            u0, rhs = rng.standard_normal(n), rng.standard_normal(n)

            def step(c):
                u, r = c.vector(n, u0), c.vector(n, rhs)
                c.smoother_step(l, u, r, False)
                return vbits(u)
            assert both(step), (name, what, l)

    n_sys = x.sys.n_dofs
    src = rng.standard_normal(n_sys) * ~np.asarray(x.h.constrained, dtype=bool)

    def vcycle(c):
        vs, vd = c.vector(n_sys, src), c.vector(n_sys)
        c.precondition(vd, vs)
        return vbits(vd)

    for kind, what in ((A.JACOBI, "Jacobi"), (A.SSOR, "SSOR")):
        for c in (a, b):
            c.set_smoother(kind, 0.5, 2)
        smooth_all(what)
    assert both(vcycle), (name, "SSOR")
    for c, res in ((a, True), (b, False)):   # SSOR in three blocks: the plan is built when the level is set
        c.set_tuning(ssor_blocks=3)
        for l in range(1, L):
            load_level(c, x, l, res, coef)
    smooth_all("SSOR, 3 blocks")
    a.close()
    b.close()


def rhs_of(c, x, resident, fill=7.0, **kw):
    n = x.rhs.n_dofs
    v = c.vector(n, np.full(n, fill))
    (c.assemble_rhs_resident if resident else c.assemble_rhs)(x.rhs, v, **kw)
    return v.download()


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_rhs_and_distribution_equal_the_siblings(name):
    A = capi()
    x = rc.case(name)
    step16 = name in rc.STEP16
    kw = dict(K_of_level=None) if step16 else {}   # (Step16: the driver passes no K_of_level, the boundary values are 0)
    a, b = resident_context(x, 1), A.Context(1)
    # with `source` given: the sibling's bits, which are the host's system_rhs
    ra, rb = rhs_of(a, x, True, **kw), rhs_of(b, x, False, **kw)
    assert np.array_equal(bits(ra), bits(rb)) and np.array_equal(bits(ra), bits(x.host_rhs))
    # with densities that stay on the device (source = NULL)
    n_cells, nq = x.rhs.source.shape
    rng = np.random.default_rng(n_cells)
    lo, h = rng.uniform(0.0, 1.0, (n_cells, 3)), np.full(n_cells, 0.25)
    atoms, q, qp = rng.uniform(0.0, 1.25, (5, 3)), rng.uniform(-1.0, 1.0, 5), rng.uniform(0.0, 1.0, (nq, 3))
    assert refused(A.ERR_INVALID, lambda: rhs_of(a, x, True, source=None, **kw), "densities")   # nothing on the device yet
    for c in (a, b):
        assert c.charge_density(lo, h, np.floor(lo), 1.0, atoms, q, 0.5, 10.0, False, qp, dens=None) is None
    da, db = rhs_of(a, x, True, source=None, **kw), rhs_of(b, x, False, source=None, **kw)
    assert np.array_equal(bits(da), bits(db)) and not np.array_equal(bits(da), bits(ra))
    # the distribution
    n = x.sys.n_dofs
    u0 = rng.standard_normal(n)
    ua, ub = a.vector(n, u0), b.vector(n, u0)
    a.distribute_constraints_resident(ua)
    b.distribute_constraints(ub, x.sys.constraint_of_dof, x.sys.line_ptr, x.sys.line_master, x.sys.line_weight, x.sys.line_inhomogeneity)
    assert np.array_equal(vbits(ua), vbits(ub)) and not np.array_equal(vbits(ua), bits(u0))
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 3. the refusals

def entries(c, x, u, v):
    """every entry that needs the tables; (name, call, needs the closed lines)"""
    lv = x.levels[1]
    return [("system", lambda: c.assemble_system_matrix_resident(x.sys.K_of_level), True),
            ("level", lambda: c.assemble_level_matrix_resident(1, lv.K), False),
            ("rhs", lambda: c.assemble_rhs_resident(x.rhs, v), True),
            ("distribute", lambda: c.distribute_constraints_resident(u), True)]


def test_refusals_and_the_state_afterwards():
    A = capi()
    x = rc.case("B3")
    n = x.sys.n_dofs
    L = len(x.levels)
    c = A.Context(L)
    u0 = np.arange(n, dtype=np.float64)
    u, v = c.vector(n, u0), c.vector(n, u0)

    def untouched():
        return np.array_equal(vbits(u), bits(u0)) and np.array_equal(vbits(v), bits(u0))

    def no_closed():
        return refused(A.ERR_INVALID, c.get_closed_constraints)

    values = x.sys.line_inhomogeneity[mtr.build(x.fc).n_hanging:]
    # before the tables exist
    assert refused(A.ERR_INVALID, lambda: c.close_constraints(values), "no mesh tables") and no_closed()
    for what, call, _ in entries(c, x, u, v):
        assert refused(A.ERR_INVALID, call, "no mesh tables"), what
    assert untouched()
    # before the close: only the level entry works
    build(c, x.fc)
    for what, call, needs_closed in entries(c, x, u, v):
        if needs_closed:
            assert refused(A.ERR_INVALID, call, "no closed constraints"), what
    assert no_closed() and untouched()
    c.assemble_level_matrix_resident(1, x.levels[1].K)
    assert c.get_level_matrix(1).n_rows == x.levels[1].n_dofs
    # a wrong n_values drops what an earlier close left
    c.close_constraints(values)
    assert c.get_closed_constraints().n_lines == len(x.sys.line_inhomogeneity)
    for wrong in (len(values) - 1, len(values) + 1, 0):
        assert refused(A.ERR_INVALID, lambda: c.close_constraints(values[:wrong] if wrong < len(values) else None, n_values=wrong), "n_values") and no_closed()
    c.close_constraints(values)
    # a wrong n_dofs, a bad level
    assert refused(A.ERR_INVALID, lambda: c.distribute_constraints_resident(u, n_dofs=n - 1), "n_dofs") and untouched()
    c.assemble_system_matrix_resident(x.sys.K_of_level)
    assert refused(A.ERR_INVALID, lambda: c.assemble_system_matrix_resident(None)) and c.get_system_matrix().n_rows == n   # the cell-matrix form: untouched
    assert refused(A.ERR_INVALID, lambda: c.assemble_level_matrix_resident(L, x.levels[1].K), "level outside the context")
    assert c.get_level_matrix(1).n_rows == x.levels[1].n_dofs
    assert refused(A.ERR_INVALID, lambda: c.assemble_level_matrix_resident(1, None)) and refused(A.ERR_INVALID, lambda: c.get_level_matrix(1))   # no operator left
    # a level the build did not have: tables of a forest with fewer levels in a context with more
    build(c, mtr.quadrant_2d())
    assert no_closed()   # a new build drops the closed lines
    for what, call, needs_closed in entries(c, x, u, v):
        if needs_closed:
            assert refused(A.ERR_INVALID, call, "no closed constraints"), what
    assert refused(A.ERR_INVALID, lambda: c.assemble_level_matrix_resident(2, np.eye(4)), "no such level")
    # device densities of the wrong size with source == NULL
    build(c, x.fc)
    c.close_constraints(values)
    assert refused(A.ERR_INVALID, lambda: c.assemble_rhs_resident(x.rhs, v, source=None), "densities") and untouched()
    # after gmg_reset
    assert c.L.gmg_reset(c.h, C.c_int(L)) == A.OK
    assert no_closed() and refused(A.ERR_INVALID, c.get_mesh_tables)
    for what, call, _ in entries(c, x, u, v):
        assert refused(A.ERR_INVALID, call, "no mesh tables"), what
    # ... unless the option asks it to keep them (what the driver's upload() does)
    build(c, x.fc)
    c.close_constraints(values)
    c.set_option("reset_keeps_mesh_tables", 1)
    assert c.L.gmg_reset(c.h, C.c_int(L)) == A.OK
    assert same_lines(c.get_closed_constraints(), x.sys)
    c.set_option("reset_keeps_mesh_tables", 0)
    c.close()


def test_unsupported_on_a_communicator():
    A = capi()
    x = rc.case("B3")
    c = A.Context(len(x.levels))
    c.comm_init(0, 1, A.Context.unique_id())
    u = c.vector(x.sys.n_dofs)
    assert refused(A.ERR_UNSUPPORTED, lambda: c.close_constraints(None, n_values=0), "communicator")
    for what, call, _ in entries(c, x, u, u):
        assert refused(A.ERR_UNSUPPORTED, call, "communicator"), what
    c.close()


def test_no_leak_over_six_rounds():
    """as tests/test_gpu_lifecycle.py: build, close, every entry, reset, six times in one context; the free device memory after
    the last round equals that after the first"""
    import torch

    x = rc.case("B3")
    L = len(x.levels)
    c = capi().Context(L)
    free = []
    for _ in range(6):
        build(c, x.fc)
        c.close_constraints(x.sys.line_inhomogeneity[c.get_mesh_tables().n_hanging:])
        load(c, x, True, False)
        assert rhs_of(c, x, True).shape == (x.sys.n_dofs,)
        u = c.vector(x.sys.n_dofs)
        c.distribute_constraints_resident(u)
        u.free()
        assert c.L.gmg_reset(c.h, C.c_int(L)) == capi().OK
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    c.close()
    print("free device memory after each round, relative to the first:", [f - free[0] for f in free])
    assert free[-1] == free[0], free


# ------------------------------------------------------------------------------------------------ 4. whole runs of the driver

SKIP_KEYS = ("solve_seconds", "build_matrices_ms")   # times
# energy_norm_error is an OpenMP reduction over the cells in the order the threads finish (postprocess_error_in_energy_norm): its
# last bits differ between two runs of one configuration.  A sum of n non-negative terms in any order, then a square root: two
# such values differ by at most (n + 2) 2^-53 relative, each from the exact one.
UNORDERED_SUMS = ("energy_norm_error",)
PREREQUISITES = dict(mesh_tables_on_device=True, system_matrix_on_device=True, level_matrices_on_device=True, rhs_from_cell_tables=True)
OTHER_KEYS_ON = dict(estimator_on_device=True, analytical_on_device=True, refinement_on_device=True, transfer_on_device=True)


def norm_lines(log):
    """the driver's log -- counts, norms, residuals, energies; it prints no times -- without the one unordered sum"""
    return [l for l in log.splitlines() if "energy norm" not in l]


def driver_runs(make, cycles):
    """the same run with the key off and on: per cycle the report, the marks, the right-hand side, the initial guess and the
    solution, and the log.  Everything but the times must be equal."""
    runs = {}
    for key in (False, True):
        p = make(key)
        out = []
        for cycle in range(cycles):
            rep = p.run_cycle(cycle, on_device=True)
            assert p.operators_resident() == key and p.mesh_tables_on_device() and p.rhs_from_cell_tables(), cycle
            out.append((rep, p.refine_flags(), p.vector("rhs"), p.vector("initial_guess"), p.vector("solution")))
        assert "Operators from resident tables" not in p.log(), p.log()   # no fallback line
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
        for i in (2, 3, 4):
            assert np.array_equal(bits(a[i]), bits(b[i])), (cycle, i)
    return runs


def golden_make(golden_dir, name, right, cycles, smoother, **more):
    S = pkg().step50

    def make(key):
        args = dict(PREREQUISITES)
        args.update(more)
        p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=cycles,
                                 r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother=smoother,
                                 refinement_estimator="Kelly", operators_from_resident_tables=key, **args))
        p.read_lammps(os.path.join(golden_dir, name))
        return p

    return make


GOLDEN_RUNS = [("atom_n1_8.data", 1.0, 3, "SSOR", {}), ("atom_n1_8.data", 1.0, 3, "SSOR", OTHER_KEYS_ON), ("atom_n3_216.data", 3.0, 2, "SSOR", {})]


@pytest.mark.parametrize("name,right,cycles,smoother,more", GOLDEN_RUNS, ids=[f"{m[0]}-{m[3]}{'-all' if m[4] else ''}" for m in GOLDEN_RUNS])
def test_adaptive_run_is_unchanged(golden_dir, name, right, cycles, smoother, more, monkeypatch):
    """the golden configurations (10 vacuum cells, Kelly marking): equal iteration counts, printed norms, residuals, thresholds,
    energies, marks, log lines, and the bits of system_rhs, of the initial guess and of the distributed solution; the driver
    holds the device's closed lines against its own in every cycle (STEP50_CHECK_RESIDENT)"""
    monkeypatch.setenv("STEP50_CHECK_RESIDENT", "1")
    runs = driver_runs(golden_make(golden_dir, name, right, cycles, smoother, **more), cycles)
    last = runs[True][0][-1][0]
    assert len(last["dofs_by_level"]) >= 2 and last["cg_iterations"] >= 1


@pytest.mark.parametrize("dim,refine", ((2, 3), (3, 2)))
def test_step16_run_is_unchanged(dim, refine, monkeypatch):
    monkeypatch.setenv("STEP50_CHECK_RESIDENT", "1")
    runs = driver_runs(lambda key: step16_problem(dim, refine, 3, operators_from_resident_tables=key, **PREREQUISITES), 3)
    assert len(runs[True][0][-1][0]["dofs_by_level"]) >= refine + 2


@pytest.mark.parametrize("missing", sorted(PREREQUISITES))
def test_a_missing_prerequisite_keeps_the_host_arrays(golden_dir, missing):
    """one line says why, once over two cycles, and the run is the one without the key"""
    why = {"mesh_tables_on_device": "the mesh tables were not formed on the device", "system_matrix_on_device": "System matrix on device is not set",
           "level_matrices_on_device": "Level matrices on device is not set", "rhs_from_cell_tables": "RHS from cell tables is not set"}[missing]
    p = golden_make(golden_dir, "atom_n1_8.data", 1.0, 2, "SSOR", **{missing: False})(True)
    q = golden_make(golden_dir, "atom_n1_8.data", 1.0, 2, "SSOR", **{missing: False})(False)
    for cycle in range(2):
        r1, r0 = p.run_cycle(cycle, on_device=True), q.run_cycle(cycle, on_device=True)
        assert not p.operators_resident() and r1["cg_iterations"] == r0["cg_iterations"]
        assert np.array_equal(bits(p.vector("rhs")), bits(q.vector("rhs"))) and np.array_equal(bits(p.vector("solution")), bits(q.vector("solution")))
    assert p.log().count(f"Operators from resident tables: not applicable ({why}), host arrays") == 1
    p.close()
    q.close()


def test_distributed_run_keeps_the_host_arrays(golden_dir):
    p = golden_make(golden_dir, "atom_n1_8.data", 1.0, 1, "SSOR")(True)
    q = golden_make(golden_dir, "atom_n1_8.data", 1.0, 1, "SSOR")(False)
    for r in (p, q):
        r.set_communicator(0, 1, capi().Context.unique_id())
    r1, r0 = p.run_cycle(0, on_device=True), q.run_cycle(0, on_device=True)
    assert not p.operators_resident() and r1["cg_iterations"] == r0["cg_iterations"]
    assert np.array_equal(bits(p.vector("rhs")), bits(q.vector("rhs"))) and np.array_equal(bits(p.vector("solution")), bits(q.vector("solution")))
    assert p.log().count("Operators from resident tables: not applicable (the run is distributed), host arrays") == 1
    p.close()
    q.close()
