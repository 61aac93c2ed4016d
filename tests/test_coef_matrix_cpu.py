"""The operators of the variable-coefficient problem (Step16: a = 5 inside r < 0.5, else 1) restated from the exported
coefficient inputs (tests/coef_matrix_reference.py) against the host driver's assembly, bit for bit, on adaptively refined 2D
and 3D meshes with hanging nodes and interface matrices; the exported coefficient values against the Step16 function evaluated
here; and the argument checks of the new entry points that need no device.  Needs no GPU."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import coef_matrix_reference as cmr
import system_matrix_reference as smr
from gpu_util import capi, pkg

#  name: (dim, global refinements, cycle) -- Kelly marking, oracle solves with the Jacobi smoother between the cycles
CASES = {"2D-c1": (2, 3, 1), "2D-c2": (2, 3, 2), "3D-g2-c1": (3, 2, 1), "3D-g3-c1": (3, 3, 1),
         "2D-c0": (2, 3, 0), "3D-g2-c0": (3, 2, 0), "3D-g3-c0": (3, 3, 0)}
REFINED = ("2D-c1", "2D-c2", "3D-g2-c1", "3D-g3-c1")
#  what the refined cases had when they were chosen: cells, hanging DoFs, cells with a = 5 / a = 1 / both at their points, mixed
#  cells that touch a hanging DoF, stored entries of the interface matrices (the levels that have one)
EXPECTED = {"2D-c1": (205, 16, (13, 187, 5), 2, [78]), "2D-c2": (223, 22, (17, 199, 7), 2, [66, 16]),
            "3D-g2-c1": (225, 117, (1, 217, 7), 1, [752]), "3D-g3-c1": (3186, 477, (23, 3135, 28), 6, [4514])}


def step16_problem(dim, refine, cycles, **kw):
    S = pkg().step50
    args = dict(left=0, right=1, problem="Step16", dim=dim, bc="Homogeneous", cycles=cycles, global_refinement=refine, smoother="Jacobi",
                refinement_estimator="Kelly")
    args.update(kw)
    return S.Problem(S.prm_text(**args))


def snapshot(p):
    """everything the comparisons need from the current cycle of p"""
    levels = [SimpleNamespace(inp=p.level_coefficient_inputs(l), host_A=p.matrix("level", l), host_I=p.matrix("edge", l)) for l in range(p.n_levels())]
    return SimpleNamespace(sys=p.system_coefficient_inputs(), host_S=p.matrix("system"), levels=levels, h=p.hierarchy(), xyz=p.dof_coordinates())


@functools.lru_cache(maxsize=None)
def _cycles(dim, refine, last):
    from oracle import gmg_oracle as go

    p = step16_problem(dim, refine, last + 1)
    out = []
    for cycle in range(last + 1):
        p.run_cycle(cycle, on_device=False)
        out.append(snapshot(p))
        if cycle < last:
            h = out[-1].h
            p.finish_cycle_with(go.OracleMG(h, smoother=go.JACOBI).solve(h.system_rhs, x0=p.vector("initial_guess"))["x"])
    p.close()
    return tuple(out)


def case(name):
    dim, refine, cycle = CASES[name]
    last = max(c for d, r, c in CASES.values() if (d, r) == (dim, refine))
    return _cycles(dim, refine, last)[cycle]


def cell_kinds(inp):
    """per cell: 5 (a = 5 at all of its points), 1 (a = 1 at all), 0 (both)"""
    cc = inp.cell_coef
    return np.where(np.all(cc == 5.0, axis=1), 5, np.where(np.all(cc == 1.0, axis=1), 1, 0))


def coverage(x):
    """(cells, hanging DoFs, (cells of kind 5, 1, mixed), mixed cells with a hanging DoF, interface entries per level)"""
    s = x.sys
    kinds = cell_kinds(s)
    n_line = np.diff(s.line_ptr)
    hanging = (s.constraint_of_dof >= 0) & (n_line[np.maximum(s.constraint_of_dof, 0)] > 0)
    mixed_hanging = int(np.sum((kinds == 0) & np.any(hanging[s.cell_dofs], axis=1)))
    return (len(kinds), int(hanging.sum()), (int(np.sum(kinds == 5)), int(np.sum(kinds == 1)), int(np.sum(kinds == 0))), mixed_hanging,
            [int(l.host_I.nnz) for l in x.levels if l.host_I.nnz])


def assert_covers(name):
    """the conditions every user of a refined case relies on; a change of the marks must not silently empty the test"""
    cells, hanging, (k5, k1, mixed), mixed_hanging, edges = coverage(case(name))
    assert k5 > 0 and k1 > 0 and mixed > 0, (name, k5, k1, mixed)
    assert hanging > 0 and mixed_hanging > 0, (name, hanging, mixed_hanging)
    assert any(e > 0 for e in edges), (name, edges)


@pytest.mark.parametrize("name", REFINED)
def test_cases_cover_what_the_comparison_is_about(name):
    assert_covers(name)
    print(name, coverage(case(name)))
    assert coverage(case(name)) == EXPECTED[name]


@pytest.mark.parametrize("name", CASES)
def test_reference_equals_host_assembly(name):
    x = case(name)
    if name in REFINED:
        assert_covers(name)
    assert x.sys.n_dofs == x.host_S.n_rows and x.sys.cell_dofs.shape[1] == 1 << x.sys.dim == x.sys.nq
    assert cmr.same_bits(cmr.assemble_system(x.sys), x.host_S), name
    for l, lv in enumerate(x.levels):
        ref = cmr.assemble_level(lv.inp)
        assert cmr.same_bits(ref.A, lv.host_A), (name, l)
        kept = cmr.pruned(lv.host_I)
        assert cmr.same_or_absent(ref.I, kept), (name, l)
        if kept is not None and kept.nnz:
            assert cmr.same_bits(ref.It, cmr.transposed(kept)), (name, l)
        else:
            assert ref.It.nnz == 0, (name, l)
        # setup_diag restated on the host's arrays
        A = lv.host_A
        rows = np.repeat(np.arange(A.n_rows), np.diff(A.rowptr))
        diag = np.zeros(A.n_rows)
        diag[rows[A.col == rows]] = A.val[A.col == rows]
        assert np.all(diag > 0.0) and np.array_equal((1.0 / diag).view(np.uint64), ref.invd.view(np.uint64)), (name, l)
        lmax = 0.0
        for r in range(A.n_rows):
            rs = 0.0
            for v in A.val[A.rowptr[r]:A.rowptr[r + 1]].tolist():
                rs += abs(v)
            lmax = max(lmax, rs / abs(float(diag[r])))
        assert lmax == ref.lmax, (name, l)


def step16(points):
    """the coefficient of the problem, include/step_50.h: 5 inside r < 0.5, else 1 -- and how far the nearest point is from
    the sphere"""
    s = np.sum(points * points, axis=-1)
    return np.where(s < 0.25, 5.0, 1.0), float(np.min(np.abs(s - 0.25)))


def gauss_points(dim):
    """the points of QGauss<dim>(2) on the unit cell, x fastest"""
    x1 = [0.5 * (1.0 - 1.0 / np.sqrt(3.0)), 0.5 * (1.0 + 1.0 / np.sqrt(3.0))]
    return np.array([[x1[(q >> d) & 1] for d in range(dim)] for q in range(1 << dim)])


@pytest.mark.parametrize("name", CASES)
def test_coefficient_values_are_the_step16_function_at_the_quadrature_points(name):
    x = case(name)
    dim = x.sys.dim
    pts = gauss_points(dim)
    tables = [(x.sys.cell_dofs, x.sys.cell_coef, x.xyz)]
    for l, lv in enumerate(x.levels):   # the level's DoFs have no coordinates of their own: through the copy lists
        xyz = np.full((lv.inp.n_dofs, 3), np.nan)
        xyz[x.h.copy_level[l]] = x.xyz[x.h.copy_global[l]]
        tables.append((lv.inp.cell_dofs, lv.inp.cell_coef, xyz))
    checked = 0
    for cd, cc, xyz in tables:
        x0, x1 = xyz[cd[:, 0], :dim], xyz[cd[:, -1], :dim]
        known = ~np.isnan(x0).any(axis=1) & ~np.isnan(x1).any(axis=1)
        if not known.any():   # (a level none of whose cells has both corners in the copy list)
            continue
        h = (x1 - x0)[:, :1]
        want, margin = step16(x0[known, None, :] + h[known, None, :] * pts[None, :, :])
        assert margin > 1e-9, margin   # no point so near the sphere that the last bit of its coordinates decides
        assert np.array_equal(cc[known], want), name
        checked += int(known.sum())
    assert checked >= len(x.sys.cell_coef)
    # G, qw and the scales: the unit cell's Laplacian comes out of them
    s = x.sys
    assert s.qw.shape == (s.nq,) and abs(s.qw.sum() - 1.0) < 1e-14 and s.G.shape == (s.nq, 1 << dim, 1 << dim)
    assert np.array_equal(s.scale_of_level, (0.5 ** np.arange(16)) ** (dim - 2))
    for l, lv in enumerate(x.levels):
        assert lv.inp.scale == s.scale_of_level[l] and np.array_equal(lv.inp.G, s.G) and np.array_equal(lv.inp.qw, s.qw)


def test_array_and_loop_cell_matrices_agree():
    x = case("3D-g2-c1")
    s = x.sys
    K = cmr.system_cell_matrices(s)
    mixed = np.flatnonzero(cell_kinds(s) == 0)
    for c in list(mixed[:3]) + [0, len(K) - 1]:
        loops = cmr.cell_matrix_loops(s.nq, s.cell_coef[c], s.G, s.qw, s.scale_of_level[s.cell_level[c]])
        assert np.array_equal(K[c].view(np.uint64), loops.view(np.uint64)), c
    rng = np.random.default_rng(5)
    G, qw = cmr.random_tables(rng, 5, 4)
    cc = cmr.random_coefficients(rng, 7, 5)
    K = cmr.cell_matrices(5, cc, G, qw, np.full(7, 0.75))
    for c in range(7):
        assert np.array_equal(K[c].view(np.uint64), cmr.cell_matrix_loops(5, cc[c], G, qw, 0.75).view(np.uint64))


def test_constant_coefficient_reproduces_the_cell_matrix_entries():
    """cell_coef = 1 and scales that are powers of two: K_c is the K_of_level of the constant-coefficient entry, bit for bit"""
    s = case("2D-c1").sys
    one = cmr.with_coefficients(s, s.nq, np.ones_like(s.cell_coef), s.G, s.qw, scale_of_level=s.scale_of_level)
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=1, mesh_size=0.25, vacuum=1, problem="GaussianCharges", dim=2, bc="Homogeneous", cycles=1, r_c=0.5,
                             global_refinement=0))
    p.run_cycle(0, on_device=False)
    K = p.system_assembly_inputs().K_of_level
    p.close()
    assert np.array_equal(cmr.system_cell_matrices(one).view(np.uint64), K[s.cell_level].view(np.uint64))


def test_null_context_is_refused():
    L = capi().load()
    assert L.gmg_assemble_system_matrix_coef(None, C.c_int(3), C.c_int64(0), C.c_int64(0), None, None, C.c_int(8), None, None, None, None, None,
                                             C.c_int64(0), None, None, None, None) == capi().ERR_INVALID
    assert L.gmg_assemble_level_matrix_coef(None, C.c_int(0), C.c_int(3), C.c_int64(0), C.c_int64(0), None, C.c_int(8), None, None, None,
                                            C.c_double(1.0), None, None) == capi().ERR_INVALID


def test_python_side_validation():
    """the binding checks shapes before the library is called (a view of a null handle would otherwise be dereferenced)"""
    ctx = capi().Context.view(C.c_void_p())
    s = case("2D-c0").sys
    args = dict(dim=2, n_dofs=s.n_dofs, cell_dofs=s.cell_dofs, cell_level=s.cell_level, nq=s.nq, cell_coef=s.cell_coef, G=s.G, qw=s.qw,
                scale_of_level=s.scale_of_level, constraint_of_dof=s.constraint_of_dof, line_ptr=s.line_ptr, line_master=s.line_master,
                line_weight=s.line_weight)
    for bad in (dict(dim=4), dict(nq=0), dict(nq=65), dict(cell_coef=s.cell_coef[:-1]), dict(G=s.G[:-1]), dict(qw=s.qw[:-1]),
                dict(scale_of_level=s.scale_of_level[:15]), dict(n_dofs=s.n_dofs + 1)):
        with pytest.raises(ValueError):
            ctx.assemble_system_matrix_coef(**dict(args, **bad))
    lv = case("2D-c0").levels[1].inp
    args = dict(level=1, dim=2, n_dofs=lv.n_dofs, cell_dofs=lv.cell_dofs, nq=lv.nq, cell_coef=lv.cell_coef, G=lv.G, qw=lv.qw, scale=lv.scale,
                dof_flags=lv.dof_flags)
    for bad in (dict(dim=4), dict(nq=0), dict(nq=65), dict(cell_coef=lv.cell_coef[:-1]), dict(G=lv.G[:-1]), dict(qw=lv.qw[:-1]),
                dict(dof_flags=lv.dof_flags[:-1])):
        with pytest.raises(ValueError):
            ctx.assemble_level_matrix_coef(**dict(args, **bad))


def test_keys_apply_to_the_variable_coefficient():
    """a cycle that does not run on the device keeps the host path and says why -- the coefficient is no reason any more"""
    q = step16_problem(2, 3, 1, system_matrix_on_device=True, level_matrices_on_device=True)
    q.run_cycle(0, on_device=False)
    log = q.log()
    assert not q.system_matrix_on_device() and not q.level_matrices_on_device()
    assert log.count("not applicable (the cycle does not run on the device)") == 2 and "coefficient varies" not in log
    assert smr.same_bits(q.matrix("system"), case("2D-c0").host_S)
    q.close()
