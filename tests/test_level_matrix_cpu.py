"""The level matrices A_l and the interface matrices I_l restated from the exported assembly inputs
(tests/level_matrix_reference.py) against the host driver's assemble_level, bit for bit, on every level of the adaptive
hierarchies A3 and B3 of tests/mg_cases.py and of a 2D problem; and what "Level matrices on device" does to a cycle that
does not run on the device.  Needs no GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import level_matrix_reference as lmr
import mg_cases
from gpu_util import capi, pkg

GOLDEN = mg_cases.GOLDEN
CASES = ("A3", "B3", "2D")
#  2D: a Gaussian charge at the origin on [-1.5, 1.5]^2, two adaptive refinements (rows per level, stored edge entries)
ROWS_2D, EDGES_2D = [169, 65, 65], [0, 72, 72]


def adaptive_problem(name, **kw):
    """the Problem of mg_cases.ADAPTIVE[name] at its last cycle, advanced on the host with the oracle's solutions exactly as
    mg_cases builds the hierarchy (which closes its Problem); kw: further prm keys"""
    from oracle import gmg_oracle as go

    vac, mesh, bc, last, rows, edges = mg_cases.ADAPTIVE[name][:6]
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=1, mesh_size=mesh, vacuum=vac, problem="GaussianCharges", dim=3, bc=bc, cycles=last + 1,
                             r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR", **kw))
    p.read_lammps(os.path.join(GOLDEN, "atom_n1_2.data"))
    for cycle in range(last + 1):
        p.run_cycle(cycle, on_device=False)
        if cycle < last:
            h = p.hierarchy()
            p.finish_cycle_with(go.OracleMG(h, smoother=go.SSOR).solve(h.system_rhs, x0=p.vector("initial_guess"))["x"])
    return p, rows, edges


def problem_2d(**kw):
    """a 2D constant-coefficient problem refined twice around the origin (the estimator is driven by a given bump)"""
    S = pkg().step50
    p = S.Problem(S.prm_text(left=-1, right=1, mesh_size=0.25, vacuum=1, problem="GaussianCharges", dim=2, bc="Homogeneous", cycles=3, r_c=0.5,
                             global_refinement=0, smoother="SSOR", **kw))
    for cycle in range(3):
        p.run_cycle(cycle, on_device=False)
        if cycle < 2:
            xy = p.dof_coordinates()
            p.finish_cycle_with(np.exp(-8.0 * (xy[:, 0] ** 2 + xy[:, 1] ** 2)))
    return p, ROWS_2D, EDGES_2D


@functools.lru_cache(maxsize=None)
def case(name):
    """namespace(levels, h): per level namespace(inp, host_A, host_I (as stored, with its zeros), ref), and the hierarchy the
    host hands to solve(); a drifting mesh fails here"""
    from types import SimpleNamespace

    p, rows, edges = problem_2d() if name == "2D" else adaptive_problem(name)
    levels = []
    for l in range(p.n_levels()):
        inp = p.level_assembly_inputs(l)
        levels.append(SimpleNamespace(inp=inp, host_A=p.matrix("level", l), host_I=p.matrix("edge", l), ref=lmr.assemble(inp)))
    h = p.hierarchy()
    p.close()
    assert [x.host_A.n_rows for x in levels] == rows, name
    assert [x.host_I.nnz for x in levels] == edges, name
    return SimpleNamespace(levels=tuple(levels), h=h)


@pytest.mark.parametrize("name", CASES)
def test_reference_equals_host_assembly(name):
    for l, x in enumerate(case(name).levels):
        assert x.inp.n_dofs == x.host_A.n_rows and x.inp.cell_dofs.shape[1] == 1 << x.inp.dim, (name, l)
        assert lmr.same_bits(x.ref.A, x.host_A), (name, l)
        kept = lmr.pruned(x.host_I)
        assert lmr.same_or_absent(x.ref.I, kept), (name, l)
        if kept is not None and kept.nnz:
            assert lmr.same_bits(x.ref.It, lmr.transposed(kept)), (name, l)
        else:
            assert x.ref.It.nnz == 0, (name, l)
        # setup_diag restated on the host's arrays
        A = x.host_A
        diag = np.zeros(A.n_rows)
        rows = np.repeat(np.arange(A.n_rows), np.diff(A.rowptr))
        on = A.col == rows
        diag[rows[on]] = A.val[on]
        assert np.all(diag > 0.0), (name, l)   # every row of a level matrix has a positive diagonal
        assert np.array_equal((1.0 / diag).view(np.uint64), x.ref.invd.view(np.uint64)), (name, l)
        lmax = 0.0
        for r in range(A.n_rows):
            rs = 0.0
            for v in A.val[A.rowptr[r]:A.rowptr[r + 1]].tolist():
                rs += abs(v)
            lmax = max(lmax, rs / abs(float(diag[r])))
        assert lmax == x.ref.lmax, (name, l)


def test_cases_cover_what_the_comparison_is_about():
    """boundary rows, refinement-edge rows, a level with an interface matrix and one without, and both dimensions: without
    them the comparisons above prove nothing"""
    seen = dict(boundary=0, edge=0, both=0, with_I=0, without_I=0, dims=set())
    for name in CASES:
        for x in case(name).levels:
            fl = x.inp.dof_flags
            seen["boundary"] += int(np.sum(fl & 1 != 0))
            seen["edge"] += int(np.sum(fl == 2))
            seen["both"] += int(np.sum(fl == 3))
            seen["with_I" if x.ref.I.nnz else "without_I"] += 1
            seen["dims"].add(x.inp.dim)
    print(seen)
    assert seen["boundary"] > 0 and seen["edge"] > 0 and seen["with_I"] > 0 and seen["without_I"] > 0, seen
    assert seen["dims"] == {2, 3}


def test_hand_built_inputs():
    """the inputs the GPU tests put through the ABI: the patch has every flag combination, the fans have the wide rows"""
    p = lmr.patch_2d()
    assert sorted(set(p.dof_flags.tolist())) == [0, 1, 2, 3]
    r = lmr.assemble(p)
    assert r.A.n_rows == 16 and lmr.same_bits(r.It, lmr.transposed(r.I))
    # rows 13 and 14 (on the edge, not on the boundary) reach the free vertices 9 and 10 below them; (13, 10) sums to 0.0 and is dropped
    assert np.diff(r.I.rowptr)[[13, 14]].tolist() == [1, 2] and r.I.nnz == 3 and r.I.col.tolist() == [9, 9, 10]
    for n_cells, width in ((100, 301), (200, 601)):
        f = lmr.fan_2d(n_cells)
        assert np.diff(lmr.assemble(f).A.rowptr)[0] == width


def test_key_defaults_to_host_assembly():
    """without the key nothing is left to the device; with it, a cycle that does not run on the device says so once and keeps
    the host path"""
    S = pkg().step50
    args = dict(left=-1, right=1, mesh_size=0.25, vacuum=1, problem="GaussianCharges", dim=2, bc="Homogeneous", cycles=1, r_c=0.5, global_refinement=0)
    p = S.Problem(S.prm_text(**args))
    p.run_cycle(0, on_device=False)
    assert not p.level_matrices_on_device() and "Level matrices on device" not in p.log()
    q = S.Problem(S.prm_text(level_matrices_on_device=True, **args))
    q.run_cycle(0, on_device=False)
    assert not q.level_matrices_on_device() and q.log().count("Level matrices on device: not applicable") == 1
    assert lmr.same_bits(p.matrix("level", 0), q.matrix("level", 0))
    assert "level_matrices_on_device" not in S.prm_text(**args) and "set Level matrices on device = true" in S.prm_text(level_matrices_on_device=True)
    p.close()
    q.close()


def test_null_context_is_refused():
    L = capi().load()
    assert L.gmg_assemble_level_matrix(None, C.c_int(0), C.c_int(3), C.c_int64(0), C.c_int64(0), None, None, None, None) == capi().ERR_INVALID
    assert L.gmg_get_level_matrix(None, C.c_int(0), C.c_int(0), None, None, None, None, None, None) == capi().ERR_INVALID


def test_python_side_validation():
    """the binding checks shapes before the library is called (a view of a null handle would otherwise be dereferenced)"""
    ctx = capi().Context.view(C.c_void_p())
    inp = lmr.patch_2d()
    args = dict(level=0, dim=2, n_dofs=inp.n_dofs, cell_dofs=inp.cell_dofs, K=inp.K, dof_flags=inp.dof_flags)
    for bad in (dict(dim=4), dict(n_dofs=inp.n_dofs + 1), dict(cell_dofs=inp.cell_dofs[:, :3]), dict(K=inp.K[:3]), dict(dof_flags=inp.dof_flags[:-1])):
        with pytest.raises(ValueError):
            ctx.assemble_level_matrix(**dict(args, **bad))
