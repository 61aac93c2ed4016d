"""gmg_assemble_system_matrix_coef and gmg_assemble_level_matrix_coef on the MI355X (csrc/gmg_assemble.hpp):
the operators of a variable coefficient formed on the device from coefficient values at the quadrature points, against the
independent restatement of tests/coef_matrix_reference.py and against the host driver's matrices, bit for bit -- on the Step16
meshes of tests/test_coef_matrix_cpu.py, with synthetic coefficients and tables on the GaussianCharges meshes, against the
cell-matrix entries for a coefficient of 1, on hand-built inputs; what the context can do afterwards against a context fed the
host's CSRs; the refusals; and whole Step16 runs of the driver with the keys off and on.  Everything goes through the C ABI."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import coef_matrix_reference as cmr
import level_matrix_reference as lmr
import system_matrix_reference as smr
import test_coef_matrix_cpu as cpu
import test_level_matrix_cpu as lcpu
from conftest import rel_close
from gpu_util import capi, pkg

pytestmark = pytest.mark.gpu


def asm_system(ctx, s, **kw):
    return ctx.assemble_system_matrix_coef(s.dim, s.n_dofs, s.cell_dofs, s.cell_level, s.nq, s.cell_coef, s.G, s.qw, s.scale_of_level,
                                           s.constraint_of_dof, s.line_ptr, s.line_master, s.line_weight, **kw)


def asm_level(ctx, level, x, **kw):
    return ctx.assemble_level_matrix_coef(level, x.dim, x.n_dofs, x.cell_dofs, x.nq, x.cell_coef, x.G, x.qw, x.scale, x.dof_flags, **kw)


def device_level(ctx, level):
    A = capi()
    return tuple(ctx.get_level_matrix(level, w) for w in (A.LEVEL_A, A.LEVEL_EDGE, A.LEVEL_EDGE_T))


def level_equals_reference(ctx, level, ref):
    A, I, It = device_level(ctx, level)
    return cmr.same_bits(A, ref.A) and cmr.same_or_absent(I, ref.I) and cmr.same_or_absent(It, ref.It)


def level_equals_host(ctx, level, host_A, host_I):
    A, I, It = device_level(ctx, level)
    kept = cmr.pruned(host_I)
    absent = kept is None or kept.nnz == 0
    return cmr.same_bits(A, host_A) and cmr.same_or_absent(I, kept) and (It.nnz == 0 if absent else cmr.same_bits(It, cmr.transposed(kept)))


def system_is_empty(ctx):
    with pytest.raises(capi().GMGError) as e:
        ctx.get_system_matrix()
    return e.value.code == capi().ERR_INVALID


def level_is_empty(ctx, level):
    with pytest.raises(capi().GMGError) as e:
        ctx.get_level_matrix(level)
    return e.value.code == capi().ERR_INVALID


def bits(v):
    return v.download().view(np.uint64)


# ------------------------------------------------------------------------------------------------ 1. the Step16 meshes

@functools.lru_cache(maxsize=None)
def step16_reference(name):
    x = cpu.case(name)
    return cmr.assemble_system(x.sys), tuple(cmr.assemble_level(lv.inp) for lv in x.levels)


@pytest.mark.parametrize("name", cpu.REFINED)
def test_step16_download_equals_host_and_reference(name):
    cpu.assert_covers(name)
    x = cpu.case(name)
    ref_S, ref_levels = step16_reference(name)
    for max_blocks in (0, 1, 3):   # by size; one workgroup; three (every kernel's grid-stride loop iterates)
        c = capi().Context(len(x.levels))
        c.set_option("assemble_max_blocks", max_blocks)
        assert asm_system(c, x.sys) >= 0.0
        dev = c.get_system_matrix()
        assert cmr.same_bits(dev, ref_S) and cmr.same_bits(dev, x.host_S), (name, max_blocks)
        for l, lv in enumerate(x.levels):
            assert asm_level(c, l, lv.inp) >= 0.0
            assert level_equals_host(c, l, lv.host_A, lv.host_I), (name, l, max_blocks)
            assert level_equals_reference(c, l, ref_levels[l]), (name, l, max_blocks)
        # the norms the driver prints, on the device's CSR: l1 and linf are sequential sums, bit-equal to sums over the host's
        l1, linf, _ = c.system_matrix_norms()
        S = x.host_S
        rows = np.repeat(np.arange(S.n_rows), np.diff(S.rowptr))
        rs, cs = np.zeros(S.n_rows), np.zeros(S.n_rows)
        np.add.at(rs, rows, np.abs(S.val))
        np.add.at(cs, S.col, np.abs(S.val))
        assert linf == rs.max() and l1 == cs.max(), (name, max_blocks)
        c.close()


# ------------------------------------------------------------------------------------------------ 2. synthetic coefficients

GAUSSIAN = ("A3", "B3", "2D")


@functools.lru_cache(maxsize=None)
def gaussian_case(name):
    """the cell tables, constraint lines and flags of the constant-coefficient hierarchies of tests/mg_cases.py (A3, B3) and of
    the 2D problem of tests/test_level_matrix_cpu.py, with the host's G, qw and scales"""
    p, rows, edges = lcpu.problem_2d() if name == "2D" else lcpu.adaptive_problem(name)
    sys_old, sys_new = p.system_assembly_inputs(), p.system_coefficient_inputs()
    levels_old = [p.level_assembly_inputs(l) for l in range(p.n_levels())]
    levels_new = [p.level_coefficient_inputs(l) for l in range(p.n_levels())]
    p.close()
    assert [x.n_dofs for x in levels_old] == rows
    assert np.sum(np.diff(sys_old.line_ptr) > 0) > 0 and sum(int(np.sum(x.dof_flags == 2)) for x in levels_old) > 0   # hanging nodes, refinement edges
    assert np.all(sys_new.cell_coef == 1.0)
    return SimpleNamespace(sys_old=sys_old, sys_new=sys_new, levels_old=levels_old, levels_new=levels_new)


def tables(cs, nq, rng):
    """(G, qw): the host's for nq == 0, else synthetic ones with nq points"""
    s = cs.sys_new
    return (s.nq, s.G, s.qw) if nq == 0 else (nq,) + cmr.random_tables(rng, nq, 1 << s.dim)


@pytest.mark.parametrize("nq", (0, 1, 5, 27))
@pytest.mark.parametrize("name", GAUSSIAN)
def test_synthetic_coefficients_equal_reference(name, nq):
    """a coefficient of its own at every point of every cell: a wrong cell or point index, or nq taken for 2^dim, shows"""
    cs = gaussian_case(name)
    if nq == 27 and cs.sys_new.dim == 2:
        nq = 9
    rng = np.random.default_rng(1000 + nq)
    n, G, qw = tables(cs, nq, rng)
    s = cs.sys_new
    inp = cmr.with_coefficients(s, n, cmr.random_coefficients(rng, len(s.cell_level), n), G, qw, scale_of_level=s.scale_of_level)
    assert np.any(inp.cell_coef < 0.0)
    c = capi().Context(len(cs.levels_new))
    asm_system(c, inp)
    assert cmr.same_bits(c.get_system_matrix(), cmr.assemble_system(inp)), (name, nq)
    for l, lv in enumerate(cs.levels_new):
        inp = cmr.with_coefficients(lv, n, cmr.random_coefficients(rng, len(lv.cell_dofs), n), G, qw, scale=lv.scale)
        asm_level(c, l, inp)
        assert level_equals_reference(c, l, cmr.assemble_level(inp)), (name, nq, l)
    c.close()


# ------------------------------------------------------------------------------------------------ 3. the old entries against the new

@pytest.mark.parametrize("name", GAUSSIAN)
def test_coefficient_one_gives_the_bits_of_the_cell_matrix_entries(name):
    cs = gaussian_case(name)
    s = cs.sys_new
    levels_used = np.unique(s.cell_level)
    scales = np.concatenate([s.scale_of_level[levels_used], [lv.scale for lv in cs.levels_new]])
    assert np.all(np.frexp(scales)[0] == 0.5), scales   # powers of two: scaling K after the sum or every term of it is the same
    a, b = capi().Context(len(cs.levels_new)), capi().Context(len(cs.levels_new))
    o = cs.sys_old
    a.assemble_system_matrix(o.dim, o.n_dofs, o.cell_dofs, o.cell_level, o.K_of_level, o.constraint_of_dof, o.line_ptr, o.line_master, o.line_weight)
    asm_system(b, s)
    assert cmr.same_bits(a.get_system_matrix(), b.get_system_matrix()), name
    for l, (old, new) in enumerate(zip(cs.levels_old, cs.levels_new)):
        a.assemble_level_matrix(l, old.dim, old.n_dofs, old.cell_dofs, old.K, old.dof_flags)
        asm_level(b, l, new)
        for u, v in zip(device_level(a, l), device_level(b, l)):
            assert cmr.same_bits(u, v), (name, l)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 4. hand-built 2D inputs

def tables_2d():
    s = cpu.case("2D-c0").sys
    return s.nq, s.G, s.qw


def coefficients_of_their_own(n_cells, nq):
    """cell c, point q: 1 + c + q / 8 -- every cell and every point its own value"""
    return 1.0 + np.arange(n_cells)[:, None] + np.arange(nq)[None, :] / 8.0


def hand_level(inp):
    nq, G, qw = tables_2d()
    return cmr.with_coefficients(inp, nq, coefficients_of_their_own(len(inp.cell_dofs), nq), G, qw, scale=1.0)


def test_quadrant_mesh_through_the_abi():
    nq, G, qw = tables_2d()
    q = smr.quadrant_mesh_2d()
    inp = cmr.with_coefficients(q, nq, coefficients_of_their_own(len(q.cell_level), nq), G, qw, scale_of_level=np.ones(16))
    c = capi().Context(1)
    asm_system(c, inp)
    dev = c.get_system_matrix()
    assert cmr.same_bits(dev, cmr.assemble_system(inp)) and dev.nnz > 0 and np.any(dev.val == 0.0)
    c.close()


@pytest.mark.parametrize("level", (0, 1))
def test_patch_and_fan(level):
    c = capi().Context(2)
    for inp in (hand_level(lmr.patch_2d()), hand_level(lmr.fan_2d(100))):   # the fan: a row of 301 columns, several LDS batches
        ref = cmr.assemble_level(inp)
        asm_level(c, level, inp)
        assert level_equals_reference(c, level, ref)
        assert ref.I.nnz > 0
    assert np.diff(ref.A.rowptr)[0] == 301
    c.close()


def test_fan_row_of_601_columns_is_unsupported():
    A = capi()
    c = A.Context(2)
    asm_level(c, 1, hand_level(lmr.patch_2d()))
    with pytest.raises(A.GMGError) as e:
        asm_level(c, 1, hand_level(lmr.fan_2d(200)))
    assert e.value.code == A.ERR_UNSUPPORTED and "512" in str(e.value) and "gmg_assemble_level_matrix_coef" in str(e.value)
    assert level_is_empty(c, 1)
    fan = hand_level(lmr.fan_2d(100))   # the context survives
    asm_level(c, 1, fan)
    assert level_equals_reference(c, 1, cmr.assemble_level(fan))
    c.close()


def test_zero_cells():
    A = capi()
    nq, G, qw = 8, np.zeros((8, 8, 8)), np.ones(8)
    c = A.Context(2)
    sys0 = SimpleNamespace(dim=3, n_dofs=5, cell_dofs=np.zeros((0, 8), dtype=np.int32), cell_level=np.zeros(0, dtype=np.uint8), nq=nq,
                           cell_coef=np.zeros((0, nq)), G=G, qw=qw, scale_of_level=np.ones(16), constraint_of_dof=-np.ones(5, dtype=np.int32),
                           line_ptr=None, line_master=None, line_weight=None)
    asm_system(c, sys0)
    m = c.get_system_matrix()
    assert m.n_rows == 5 and m.nnz == 0 and np.array_equal(m.rowptr, np.zeros(6, dtype=np.int64))
    assert c.system_matrix_norms() == (0.0, 0.0, 0.0)
    lv0 = SimpleNamespace(dim=3, n_dofs=5, cell_dofs=np.zeros((0, 8), dtype=np.int32), nq=nq, cell_coef=np.zeros((0, nq)), G=G, qw=qw, scale=1.0,
                          dof_flags=np.zeros(5, dtype=np.uint8))
    old = SimpleNamespace(dim=3, n_dofs=5, cell_dofs=lv0.cell_dofs, K=np.zeros((8, 8)), dof_flags=lv0.dof_flags)
    b = A.Context(2)
    for level in (0, 1):   # whatever the cell-matrix entry makes of no cells
        def outcome(f):
            try:
                f()
                return "ok"
            except A.GMGError as e:
                return e.code
        got = outcome(lambda: asm_level(c, level, lv0))
        assert got == outcome(lambda: b.assemble_level_matrix(level, old.dim, old.n_dofs, old.cell_dofs, old.K, old.dof_flags)), (level, got)
        if got == "ok":
            for w in (A.LEVEL_A, A.LEVEL_EDGE, A.LEVEL_EDGE_T):
                m = c.get_level_matrix(level, w)
                assert m.n_rows == 5 and m.nnz == 0
    c.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 5. the context afterwards

def load(c, x, on_device):
    """everything solve() consumes: the operators by the _coef entries, or the host's CSRs"""
    h = x.h
    if on_device:
        asm_system(c, x.sys)
    else:
        c.set_system_matrix(h.system_matrix)
    for l in range(len(x.levels)):
        reload_level(c, x, l, on_device)
        c.set_copy_indices(l, h.copy_global[l], h.copy_level[l])
    for l, P in enumerate(h.prolongations):
        c.set_prolongation(l, P)


def reload_level(c, x, l, on_device):
    if on_device:
        asm_level(c, l, x.levels[l].inp)
        return
    c.set_level_matrix(l, x.h.level_matrices[l])
    I = x.h.edge_matrices[l]
    if I is not None and I.nnz > 0:
        c.set_edge_matrix(l, I)


@pytest.mark.parametrize("name", ("2D-c2", "3D-g2-c1"))
def test_context_equals_one_fed_the_host_matrices(name):
    """SpMV on the system matrix and on every level, one step of every smoother on the levels that carry one (Jacobi pins
    invd, Chebyshev cheb_lmax, SSOR the plan, in 1 and 3 blocks) and whole V-cycles (I_l and I_l^T) -- identical bits"""
    A = capi()
    cpu.assert_covers(name)
    x = cpu.case(name)
    L = len(x.levels)
    a, b = A.Context(L), A.Context(L)
    load(a, x, True)
    load(b, x, False)
    rng = np.random.default_rng(L)

    def both(f):
        return np.array_equal(f(a), f(b))

    sizes = [(A.SYSTEM, x.sys.n_dofs)] + [(l, lv.inp.n_dofs) for l, lv in enumerate(x.levels)]
    for which, n in sizes:
        v = rng.standard_normal(n)

        def spmv(c):
            vx, vy = c.vector(n, v), c.vector(n)
            c.spmv(which, vy, vx)
            return bits(vy)
        assert both(spmv), (name, "spmv", which)

    def smooth_all(what):
        for l in range(1, L):
            n = x.levels[l].inp.n_dofs
            u0, rhs = rng.standard_normal(n), rng.standard_normal(n)
            for from_zero in (True, False):
                def step(c):
                    u, r = c.vector(n, u0), c.vector(n, rhs)
                    c.smoother_step(l, u, r, from_zero)
                    return bits(u)
                assert both(step), (name, what, l, from_zero)

    n_sys = x.sys.n_dofs
    src = rng.standard_normal(n_sys) * ~np.asarray(x.h.constrained, dtype=bool)

    def vcycle(c):
        vs, vd = c.vector(n_sys, src), c.vector(n_sys)
        c.precondition(vd, vs)
        return bits(vd)

    for kind, what in ((A.JACOBI, "Jacobi"), (A.CHEBYSHEV, "Chebyshev"), (A.SSOR, "SSOR")):
        for c in (a, b):
            c.set_smoother(kind, 0.5, 2, cheb_degree=3)
        smooth_all(what)
        assert both(vcycle), (name, what)
    for c, dev in ((a, True), (b, False)):   # SSOR in three blocks: the plan is built when the level is set
        c.set_tuning(ssor_blocks=3)
        for l in range(1, L):
            reload_level(c, x, l, dev)
    smooth_all("SSOR, 3 blocks")
    assert both(vcycle), (name, "SSOR, 3 blocks")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 6. refusals and lifecycle

def changed(good, **kw):
    d = dict(vars(good))
    d.update(kw)
    return SimpleNamespace(**d)


NONE = np.zeros(0)   # the binding passes an empty array as NULL


def test_refused_arguments_leave_no_operator():
    A = capi()
    x = cpu.case("2D-c1")
    s, lv = x.sys, x.levels[1].inp
    ref_S, ref_levels = step16_reference("2D-c1")
    c = A.Context(len(x.levels))
    bad_system = {"nq 0": changed(s, nq=0), "nq 65": changed(s, nq=65), "nq -1": changed(s, nq=-1), "null cell_coef": changed(s, cell_coef=NONE),
                  "null G": changed(s, G=NONE), "null qw": changed(s, qw=NONE), "null scale": changed(s, scale_of_level=NONE),
                  "dim": changed(s, dim=4), "null cell_dofs": changed(s, cell_dofs=np.zeros((0, 4), dtype=np.int32))}
    for what, inp in bad_system.items():
        asm_system(c, s)
        with pytest.raises(A.GMGError) as e:
            asm_system(c, inp, validate=False)
        assert e.value.code == A.ERR_INVALID and "gmg_assemble_system_matrix_coef" in str(e.value), what
        assert system_is_empty(c), what
    asm_system(c, s)
    assert cmr.same_bits(c.get_system_matrix(), ref_S)
    bad_level = {"nq 0": changed(lv, nq=0), "nq 65": changed(lv, nq=65), "null cell_coef": changed(lv, cell_coef=NONE), "null G": changed(lv, G=NONE),
                 "null qw": changed(lv, qw=NONE), "dim": changed(lv, dim=1), "null flags": changed(lv, dof_flags=np.zeros(0, dtype=np.uint8))}
    for what, inp in bad_level.items():
        asm_level(c, 1, lv)
        with pytest.raises(A.GMGError) as e:
            asm_level(c, 1, inp, validate=False)
        assert e.value.code == A.ERR_INVALID and "gmg_assemble_level_matrix_coef" in str(e.value), what
        assert level_is_empty(c, 1), what
    asm_level(c, 1, lv)
    with pytest.raises(A.GMGError) as e:   # no such level: nothing is touched
        asm_level(c, len(x.levels), lv)
    assert e.value.code == A.ERR_INVALID and level_equals_reference(c, 1, ref_levels[1])
    # reset, then a second assembly
    assert c.L.gmg_reset(c.h, C.c_int(len(x.levels))) == A.OK
    assert system_is_empty(c) and level_is_empty(c, 1)
    asm_system(c, s)
    asm_level(c, 1, lv)
    assert cmr.same_bits(c.get_system_matrix(), ref_S) and level_equals_reference(c, 1, ref_levels[1])
    c.close()


def test_unsupported_on_a_communicator():
    A = capi()
    x = cpu.case("2D-c1")
    c = A.Context(len(x.levels))
    c.comm_init(0, 1, A.Context.unique_id())
    with pytest.raises(A.GMGError) as e:
        asm_system(c, x.sys)
    assert e.value.code == A.ERR_UNSUPPORTED and system_is_empty(c)
    for level in (0, 1):
        with pytest.raises(A.GMGError) as e:
            asm_level(c, level, x.levels[level].inp)
        assert e.value.code == A.ERR_UNSUPPORTED and level_is_empty(c, level)
    c.close()


# ------------------------------------------------------------------------------------------------ 7. driver runs

REPORT_KEYS = ("cg_iterations", "coarse_iterations", "starting_value", "convergence_value", "matrix_l1", "matrix_linf", "dofs", "active_cells",
               "rhs_l2", "sol_l1", "sol_l2", "sol_linf")
KEYS_ON = dict(system_matrix_on_device=True, level_matrices_on_device=True)
ALL_ON = dict(KEYS_ON, estimator_on_device=True, transfer_on_device=True)


@pytest.mark.parametrize("smoother", ("SSOR", "Jacobi"))
@pytest.mark.parametrize("dim,refine", ((2, 3), (3, 2)))
def test_step16_run_is_unchanged(dim, refine, smoother):
    """three adaptive cycles of the variable-coefficient problem with both keys off, on, and on with the estimator and the
    transfers on the device as well: the same iteration counts, printed norms, residuals and refinement marks; with the keys
    no operator is assembled on the host, and what the device holds is what the host assembles when asked"""
    runs = []
    for keys in (dict(), KEYS_ON, ALL_ON):
        p = cpu.step16_problem(dim, refine, 3, smoother=smoother, **keys)
        out = []
        for cycle in range(3):
            rep = p.run_cycle(cycle, on_device=True)
            assert p.system_matrix_on_device() == p.level_matrices_on_device() == bool(keys)
            out.append((rep, p.refine_flags()))
            if keys:
                assert cmr.same_bits(p.device_system_matrix(), p.matrix("system")), cycle
                for l in range(p.n_levels()):   # level 0 too: it is no lattice operator here
                    A, I, It = (p.device_level_matrix(l, w) for w in ("level", "edge", "edge_t"))
                    kept = cmr.pruned(p.matrix("edge", l))
                    assert cmr.same_bits(A, p.matrix("level", l)) and cmr.same_or_absent(I, kept), (cycle, l)
                    assert It.nnz == I.nnz and (I.nnz == 0 or cmr.same_bits(It, cmr.transposed(kept))), (cycle, l)
        if keys:
            assert "not applicable" not in p.log(), p.log()
        runs.append(out)
        p.close()
    assert len(runs[0][-1][0]["dofs_by_level"]) > refine + 1   # the mesh was refined
    for other in runs[1:]:
        for cycle, ((r0, f0), (r1, f1)) in enumerate(zip(runs[0], other)):
            for k in REPORT_KEYS:
                assert r0[k] == r1[k], (cycle, k, r0[k], r1[k])
            assert np.array_equal(f0, f1), cycle


@pytest.mark.parametrize("dim,refine", ((2, 3), (3, 2)))
def test_inhomogeneous_dirichlet_terms_without_a_host_matrix(dim, refine):
    """the right-hand-side pass forms the inhomogeneous Dirichlet terms from the host's cell matrices whether or not the
    system matrix is assembled on the host: the same right-hand side and the same solve with the keys on.  (Two charges give
    the boundary values a dipole; the domain is moved off the origin, where that potential is singular.)"""
    reps = []
    for keys in (dict(), KEYS_ON):
        p = cpu.step16_problem(dim, refine, 1, bc="Inhomogeneous", left=0.25, right=1.25, **keys)
        p.set_atoms([1.0, -1.0], [[0.5, 0.5, 0.5 if dim == 3 else 0.0], [0.9, 0.7, 0.6 if dim == 3 else 0.0]])
        reps.append((p.run_cycle(0, on_device=True), p.vector("rhs"), p.constraint_inhomogeneities()))
        assert p.system_matrix_on_device() == p.level_matrices_on_device() == bool(keys)
        p.close()
    (r0, b0, g0), (r1, b1, g1) = reps
    assert np.count_nonzero(g0) > 0 and np.array_equal(g0, g1)
    assert np.array_equal(b0.view(np.uint64), b1.view(np.uint64))
    for k in REPORT_KEYS:
        assert r0[k] == r1[k], k


@pytest.mark.parametrize("key,dim,iterations", (("tests_3D/step-16.mpirun=1", 3, 8), ("tests_2D/step-16.mpirun=1", 2, 7)))
def test_golden_cycle0_with_the_keys(golden, key, dim, iterations):
    """cycle 0 of the reference's Step16 logs with every operator formed on the device: the printed iteration count and
    solution norms"""
    g = golden[key]["runs"][0]["cycles"][0]
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=1, problem="Step16", dim=dim, bc="Homogeneous", cycles=1, global_refinement=4, smoother="Jacobi", **KEYS_ON))
    r = p.run_cycle(0)
    assert p.system_matrix_on_device() and p.level_matrices_on_device() and "not applicable" not in p.log()
    assert r["cg_iterations"] == g["cg_iterations"] == iterations
    for k in ("sol_l1", "sol_l2", "sol_linf"):
        assert rel_close(r[k], g[k], 6), k
    assert r["dofs_by_level"] == g["dofs_by_level"] and r["active_cells"] == g["active_cells"]
    p.close()
