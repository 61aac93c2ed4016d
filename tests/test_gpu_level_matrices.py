"""gmg_assemble_level_matrix and gmg_get_level_matrix on the MI355X (csrc/gmg_assemble.hpp) against the
host driver's assemble_level and the independent restatement of tests/level_matrix_reference.py, bit for bit; the level
they leave behind against gmg_set_level_matrix + gmg_set_edge_matrix with the host CSR (SpMV, the three smoothers, a whole
V-cycle); hand-built inputs, refusals and lifecycle through the ABI; and whole adaptive runs with "Level matrices on device"
against the same runs without it."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import level_matrix_reference as lmr
from gpu_util import capi, pkg
from test_level_matrix_cpu import CASES, case

pytestmark = pytest.mark.gpu


def assemble(ctx, level, inp, **kw):
    return ctx.assemble_level_matrix(level, inp.dim, inp.n_dofs, inp.cell_dofs, inp.K, inp.dof_flags, **kw)


def device_matrices(ctx, level):
    A = capi()
    return tuple(ctx.get_level_matrix(level, w) for w in (A.LEVEL_A, A.LEVEL_EDGE, A.LEVEL_EDGE_T))


def equals_reference(ctx, level, ref):
    A, I, It = device_matrices(ctx, level)
    return lmr.same_bits(A, ref.A) and lmr.same_or_absent(I, ref.I) and lmr.same_or_absent(It, ref.It)


def equals_host(ctx, level, host_A, host_I):
    A, I, It = device_matrices(ctx, level)
    kept = lmr.pruned(host_I)
    absent = kept is None or kept.nnz == 0
    return lmr.same_bits(A, host_A) and lmr.same_or_absent(I, kept) and (It.nnz == 0 if absent else lmr.same_bits(It, lmr.transposed(kept)))


def bits(v):
    return v.download().view(np.uint64)


def is_empty(ctx, level):
    """the level holds no operator: gmg_get_level_matrix refuses it"""
    with pytest.raises(capi().GMGError) as e:
        ctx.get_level_matrix(level)
    return e.value.code == capi().ERR_INVALID


# ------------------------------------------------------------------------------------------------ the hierarchies, level by level

@pytest.mark.parametrize("name", CASES)
def test_download_equals_host_and_reference(name):
    levels = case(name).levels
    for max_blocks in (0, 1, 3):   # by size; one workgroup; three (every kernel's grid-stride loop iterates)
        c = capi().Context(len(levels))
        c.set_option("assemble_max_blocks", max_blocks)
        for l, x in enumerate(levels):
            ms = assemble(c, l, x.inp)
            assert ms >= 0.0
            assert equals_host(c, l, x.host_A, x.host_I), (name, l, max_blocks)
            assert equals_reference(c, l, x.ref), (name, l, max_blocks)
        c.close()


def load(c, h, levels=None):
    """everything solve() consumes; levels given: A_l and I_l by gmg_assemble_level_matrix, else the host CSR"""
    c.set_system_matrix(h.system_matrix)
    for l, A in enumerate(h.level_matrices):
        reload_level(c, h, l, levels)
        c.set_copy_indices(l, h.copy_global[l], h.copy_level[l])
    for l, P in enumerate(h.prolongations):
        c.set_prolongation(l, P)


def reload_level(c, h, l, levels):
    if levels is not None:
        assemble(c, l, levels[l].inp)
        return
    c.set_level_matrix(l, h.level_matrices[l])
    I = h.edge_matrices[l]
    if I is not None and I.nnz > 0:
        c.set_edge_matrix(l, I)


def given_bounds(n):
    """a caller-given partition with an empty block and a one-row block"""
    return [0, n // 3, n // 3, n // 3 + 1, n // 2 + 5, n]


@pytest.mark.parametrize("name", CASES)
def test_level_equals_the_uploaded_host_matrices(name):
    """a context whose levels the device assembled against one fed the host CSR: SpMV on every level, one step of every
    smoother on the levels that carry one (Jacobi pins invd, Chebyshev pins cheb_lmax, SSOR the plan), and whole V-cycles
    (which pin I_l and I_l^T) -- identical bits"""
    A = capi()
    cs = case(name)
    h, levels = cs.h, cs.levels
    L = len(levels)
    a, b = A.Context(L), A.Context(L)
    load(a, h, levels)
    load(b, h)
    rng = np.random.default_rng(L)

    def both(f):
        u, v = f(a), f(b)
        return np.array_equal(u, v)

    def smooth_all(what):
        for l in range(1, L):
            n = levels[l].inp.n_dofs
            u0, rhs = rng.standard_normal(n), rng.standard_normal(n)
            for from_zero in (True, False):
                def step(c):
                    u, r = c.vector(n, u0), c.vector(n, rhs)
                    c.smoother_step(l, u, r, from_zero)
                    return bits(u)
                assert both(step), (name, what, l, from_zero)

    for l in range(L):
        n = levels[l].inp.n_dofs
        x = rng.standard_normal(n)

        def spmv(c):
            vx, vy = c.vector(n, x), c.vector(n)
            c.spmv(l, vy, vx)
            return bits(vy)
        assert both(spmv), (name, "spmv", l)
    n_sys = h.system_matrix.n_rows
    src = rng.standard_normal(n_sys) * ~np.asarray(h.constrained, dtype=bool)

    def vcycle(c):
        vs, vd = c.vector(n_sys, src), c.vector(n_sys)
        c.precondition(vd, vs)
        return bits(vd)

    for kind, what in ((A.JACOBI, "Jacobi"), (A.CHEBYSHEV, "Chebyshev"), (A.SSOR, "SSOR")):
        for c in (a, b):
            c.set_smoother(kind, 0.5, 2, cheb_degree=3)
        smooth_all(what)
        assert both(vcycle), (name, what)
    # SSOR in three blocks, then on caller-given block rows: the plan is built when the level is set
    for c, lv in ((a, levels), (b, None)):
        c.set_tuning(ssor_blocks=3)
        for l in range(1, L):
            reload_level(c, h, l, lv)
    smooth_all("SSOR, 3 blocks")
    assert both(vcycle), (name, "SSOR, 3 blocks")
    for c, lv in ((a, levels), (b, None)):
        for l in range(1, L):
            c.set_ssor_block_rows(l, given_bounds(levels[l].inp.n_dofs))
            reload_level(c, h, l, lv)
        for l in range(1, L):
            assert np.array_equal(c.get_ssor_partition(l)[0], given_bounds(levels[l].inp.n_dofs))
    smooth_all("SSOR, given rows")
    # block rows that do not end at n_dofs are refused as gmg_set_level_matrix refuses them, and the level is left empty
    a.set_ssor_block_rows(1, [0, 5, levels[1].inp.n_dofs - 1])
    with pytest.raises(A.GMGError) as e:
        assemble(a, 1, levels[1].inp)
    assert e.value.code == A.ERR_INVALID and is_empty(a, 1)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ hand-built inputs through the ABI

def against_reference_context(inp, level):
    """assemble inp on `level` of a two-level context; the download against the reference, and SpMV, Jacobi and Chebyshev
    against a context that was handed the reference's matrices"""
    A = capi()
    ref = lmr.assemble(inp)
    a, b = A.Context(2), A.Context(2)
    assemble(a, level, inp)
    assert equals_reference(a, level, ref)
    b.set_level_matrix(level, ref.A)
    if ref.I.nnz:
        b.set_edge_matrix(level, ref.I)
    n = inp.n_dofs
    x, rhs = np.cos(np.arange(n) * 0.37) + 0.25, np.sin(np.arange(n) * 0.11)
    out = []
    for c in (a, b):
        vx, vy = c.vector(n, x), c.vector(n)
        c.spmv(level, vy, vx)
        got = [bits(vy)]
        for kind in (A.JACOBI, A.CHEBYSHEV) + ((A.SSOR,) if level > 0 else ()):
            c.set_smoother(kind, 0.5, 2, cheb_degree=3)
            u, r = c.vector(n, x), c.vector(n, rhs)
            c.smoother_step(level, u, r, False)
            got.append(bits(u))
        out.append(got)
        c.close()
    assert all(np.array_equal(u, v) for u, v in zip(*out))
    return ref


@pytest.mark.parametrize("level", (0, 1))
def test_patch_with_mixed_flags(level):
    ref = against_reference_context(lmr.patch_2d(), level)
    assert ref.I.nnz == 3 and np.any(ref.A.val == 0.0)   # a dropped zero sum; flagged rows keep their pattern as stored zeros


def test_fan_row_of_301_columns():
    """100 cells around DoF 0: its row is collected in several LDS batches and ranked by all 64 lanes several times"""
    ref = against_reference_context(lmr.fan_2d(100), 1)
    assert np.diff(ref.A.rowptr)[0] == 301 and ref.I.nnz > 64


def test_fan_row_of_601_columns_is_unsupported():
    A = capi()
    c = A.Context(2)
    assemble(c, 1, lmr.patch_2d())
    with pytest.raises(A.GMGError) as e:
        assemble(c, 1, lmr.fan_2d(200))
    assert e.value.code == A.ERR_UNSUPPORTED and "512" in str(e.value)
    assert is_empty(c, 1)
    assemble(c, 1, lmr.fan_2d(100))   # the context survives
    assert equals_reference(c, 1, lmr.assemble(lmr.fan_2d(100)))
    c.close()


# ------------------------------------------------------------------------------------------------ refusals and lifecycle

def test_invalid_arguments_are_refused_and_leave_the_level_empty():
    A = capi()
    c = A.Context(2)
    good = lmr.patch_2d()
    ref = lmr.assemble(good)

    def changed(**kw):
        d = dict(vars(good))
        d.update(kw)
        return SimpleNamespace(**d)

    def with_entry(a, i, v):
        a = np.array(a)
        a.reshape(-1)[i] = v
        return a

    bad = {
        "dim": (1, changed(dim=4)),
        "level above": (2, good),
        "level below": (-1, good),
        "dof below": (1, changed(cell_dofs=with_entry(good.cell_dofs, 5, -1))),
        "dof above": (1, changed(cell_dofs=with_entry(good.cell_dofs, 5, good.n_dofs))),
        "flag bits": (1, changed(dof_flags=with_entry(good.dof_flags, 3, 4))),
        "null flags": (1, changed(dof_flags=np.zeros(0, dtype=np.uint8))),
        "null K": (1, changed(K=np.zeros(0))),
        "negative n_dofs": (1, changed(n_dofs=-1, dof_flags=np.zeros(0, dtype=np.uint8), cell_dofs=np.zeros((0, 4), dtype=np.int32))),
    }
    for what, (level, inp) in bad.items():
        assemble(c, 1, good)
        with pytest.raises(A.GMGError) as e:
            assemble(c, level, inp, validate=False)
        assert e.value.code == A.ERR_INVALID, what
        if 0 <= level < 2:
            assert "gmg_assemble_level_matrix" in str(e.value) and is_empty(c, level), what
        else:
            assert equals_reference(c, 1, ref), what   # no such level: nothing was touched
    # a negative cell count and a NULL cell table of nonzero length: only through the raw entry
    fl, K = np.ascontiguousarray(good.dof_flags), np.ascontiguousarray(good.K)
    for n_cells in (-1, 9):
        assemble(c, 1, good)
        rc = c.L.gmg_assemble_level_matrix(c.h, C.c_int(1), C.c_int(2), C.c_int64(good.n_dofs), C.c_int64(n_cells), None,
                                           K.ctypes.data_as(C.POINTER(C.c_double)), fl.ctypes.data_as(C.POINTER(C.c_uint8)), None)
        assert rc == A.ERR_INVALID and is_empty(c, 1), n_cells
    with pytest.raises(A.GMGError) as e:
        c.get_level_matrix(1, 3)
    assert e.value.code == A.ERR_INVALID
    assemble(c, 1, good)
    assert equals_reference(c, 1, ref)
    c.close()


def test_unsupported_on_a_communicator():
    A = capi()
    c = A.Context(2)
    c.comm_init(0, 1, A.Context.unique_id())
    for level in (0, 1):
        with pytest.raises(A.GMGError) as e:
            assemble(c, level, lmr.patch_2d())
        assert e.value.code == A.ERR_UNSUPPORTED
    c.close()


def test_reset_then_another_level():
    A = capi()
    c = A.Context(1)
    assemble(c, 0, lmr.patch_2d())
    assert c.L.gmg_reset(c.h, C.c_int(2)) == A.OK
    assert is_empty(c, 0) and is_empty(c, 1)
    fan = lmr.fan_2d(100)
    assemble(c, 1, fan)
    assert equals_reference(c, 1, lmr.assemble(fan)) and is_empty(c, 0)
    c.close()


@pytest.mark.parametrize("level", (0, 1))
def test_zero_cells(level):
    """no cells: n_dofs empty rows, and whatever gmg_set_level_matrix makes of the same empty matrix"""
    A = capi()
    empty = SimpleNamespace(dim=3, n_dofs=5, cell_dofs=np.zeros((0, 8), dtype=np.int32), K=np.zeros((8, 8)), dof_flags=np.zeros(5, dtype=np.uint8))
    csr = SimpleNamespace(n_rows=5, n_cols=5, nnz=0, rowptr=np.zeros(6, dtype=np.int64), col=np.zeros(0, dtype=np.int32), val=np.zeros(0))
    x = np.arange(5) + 1.0

    def outcome(c, set_level):
        """the error code of the first call that fails, or the bits an SpMV with the level leaves"""
        try:
            set_level(c)
            vx, vy = c.vector(5, x), c.vector(5, x)
            c.spmv(level, vy, vx)
            return ("ok", bits(vy).tolist())
        except A.GMGError as e:
            return ("error", e.code)

    a, b = A.Context(2), A.Context(2)
    got = outcome(a, lambda c: assemble(c, level, empty))
    assert got == outcome(b, lambda c: c.set_level_matrix(level, csr)), got
    for w in (A.LEVEL_A, A.LEVEL_EDGE, A.LEVEL_EDGE_T):
        m = a.get_level_matrix(level, w)
        assert m.n_rows == 5 and m.n_cols == 5 and m.nnz == 0 and np.array_equal(m.rowptr, np.zeros(6, dtype=np.int64))
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ whole adaptive runs

ALL_ON = dict(system_matrix_on_device=True, estimator_on_device=True, coarse_solver="direct")
END_TO_END = [("atom_n1_8.data", 1.0, 3, "SSOR", {}), ("atom_n3_216.data", 3.0, 2, "SSOR", {}), ("atom_n1_8.data", 1.0, 3, "Jacobi", {}),
              ("atom_n1_8.data", 1.0, 3, "Chebyshev", {}), ("atom_n1_8.data", 1.0, 3, "SSOR", ALL_ON)]
REPORT_KEYS = ("cg_iterations", "coarse_iterations", "starting_value", "convergence_value", "matrix_l1", "matrix_linf", "dofs", "active_cells",
               "rhs_l2", "sol_l1", "sol_l2", "sol_linf")


def adaptive_runs(make, cycles, lattice0):
    """the same run with and without the key: per cycle (report, refinement marks).  lattice0: level 0 keeps
    gmg_set_level_matrix_lattice, which leaves no CSR on the device"""
    runs = {}
    for key in (False, True):
        p = make(key)
        out = []
        for cycle in range(cycles):
            rep = p.run_cycle(cycle, on_device=True)
            assert p.level_matrices_on_device() == key
            out.append((rep, p.refine_flags()))
            if key:   # what the device holds against the host's assembly on demand
                for l in range(p.n_levels()):
                    if l == 0 and lattice0:
                        with pytest.raises(capi().GMGError) as e:
                            p.device_level_matrix(0, "level")
                        assert e.value.code == capi().ERR_UNSUPPORTED
                        continue
                    dev = [p.device_level_matrix(l, w) for w in ("level", "edge", "edge_t")]
                    kept = lmr.pruned(p.matrix("edge", l))
                    assert lmr.same_bits(dev[0], p.matrix("level", l)) and lmr.same_or_absent(dev[1], kept), (cycle, l)
                    assert dev[2].nnz == dev[1].nnz and (dev[1].nnz == 0 or lmr.same_bits(dev[2], lmr.transposed(kept))), (cycle, l)
        if key:
            assert "not applicable" not in p.log(), p.log()
        runs[key] = out
        p.close()
    for cycle, ((r0, f0), (r1, f1)) in enumerate(zip(runs[False], runs[True])):
        for k in REPORT_KEYS:
            assert r0[k] == r1[k], (cycle, k, r0[k], r1[k])
        assert np.array_equal(f0, f1), cycle
    return runs


@pytest.mark.parametrize("name,right,cycles,smoother,more", END_TO_END, ids=[f"{m[0]}-{m[3]}{'-all' if m[4] else ''}" for m in END_TO_END])
def test_adaptive_run_is_unchanged(golden_dir, name, right, cycles, smoother, more):
    """the golden configurations (10 vacuum cells, Kelly marking) with and without the key: the same iteration counts (outer and
    coarse), the same printed residuals and norms, the same refinement marks"""
    S = pkg().step50

    def make(key):
        p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous",
                                 cycles=cycles, r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother=smoother,
                                 refinement_estimator="Kelly", level_matrices_on_device=key, **more))
        p.read_lammps(os.path.join(golden_dir, name))
        return p

    runs = adaptive_runs(make, cycles, True)
    assert len(runs[True][-1][0]["dofs_by_level"]) >= 2   # the mesh was refined: levels >= 1 went through the new entry


def test_adaptive_run_2d_is_unchanged():
    """2D: level 0 is no lattice operator for the device, so it goes through gmg_assemble_level_matrix as well"""
    S = pkg().step50

    def make(key):
        return S.Problem(S.prm_text(left=-1, right=1, mesh_size=0.25, vacuum=1, problem="GaussianCharges", dim=2, bc="Homogeneous", cycles=3,
                                    r_c=0.5, global_refinement=0, smoother="SSOR", refinement_estimator="Kelly", level_matrices_on_device=key))

    runs = adaptive_runs(make, 3, False)
    assert len(runs[True][-1][0]["dofs_by_level"]) >= 2
