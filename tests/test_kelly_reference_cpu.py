"""tests/kelly_reference.py against the host loops of the driver (estimate_error_and_mark_cells) on adaptively refined
golden meshes, through the exported inputs of gmg_estimate_error: the numpy restatement bit for bit, the 50-digit
evaluation within the derived bound; the closed form that pins ng = degree + 1; and what needs no device of the new entry
point and prm key."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import kelly_reference as kr
from gpu_util import capi, pkg

# the golden atom files on a small box: 2 vacuum cells around the atoms, mesh size 0.25
GOLDEN = [("atom_n1_8.data", 1.0, 3), ("atom_n3_216.data", 3.0, 2), ("atom_n5_1000.data", 5.0, 3)]
MP_SLOTS = 150  # slots of every kind evaluated at 50 digits per cycle (evenly spread), besides the cells near the threshold


def problem(golden_dir, name, right, cycles, rule, **kw):
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=2, problem="GaussianCharges", dim=3, bc="Exact", cycles=cycles,
                             r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR",
                             refinement_estimator=rule, **kw))
    p.read_lammps(os.path.join(golden_dir, name))
    return p


def stand_in_solution(p):
    """a solution-like vector (no solve: the estimator takes any u): the screened potential of the atoms plus a ripple"""
    q, x = p.atoms()
    X = p.dof_coordinates()
    u = np.zeros(len(X))
    for qi, xi in zip(q[:64], x[:64]):
        u += qi * np.exp(-((X - xi) ** 2).sum(1) / 0.6)
    return u + 0.02 * np.sin(3.0 * X[:, 0] + 1.0) * np.cos(2.0 * X[:, 1]) * np.cos(1.5 * X[:, 2] + 0.5)


def exported(p):
    k, r, _, _ = p.estimator_components()
    return SimpleNamespace(face_int=p.face_integrals(), kelly_sq=k, residual_sq=r, eta=p.error_per_cell(), mark=p.marks(),
                           threshold=p.report()["refine_threshold"], n_marked=int(p.marks().sum()))


@pytest.mark.parametrize("rule", ["Kelly + residual", "Kelly"])
@pytest.mark.parametrize("name,right,cycles", GOLDEN, ids=[m[0] for m in GOLDEN])
def test_reference_equals_host_loop(golden_dir, name, right, cycles, rule):
    p = problem(golden_dir, name, right, cycles, rule)
    seen = np.zeros(4, dtype=np.int64)
    worst = 0.0
    for cycle in range(cycles):
        p.run_cycle(cycle, on_device=False)
        p.finish_cycle_with(stand_in_solution(p))
        first = exported(p)
        p.estimate(on_device=False)
        host = exported(p)
        assert kr.same_bits(host, first) == [] and not p.estimated_on_device()
        inp = p.estimator_inputs()
        assert inp.residual == (2 if rule == "Kelly" else 1) and not inp.dens_resident and inp.ng == 2 and inp.nq == 8
        u = p.vector("solution")
        ref = kr.estimate(inp, u)
        assert kr.same_bits(host, ref) == [], cycle
        seen += np.bincount(inp.face_kind.ravel(), minlength=4)
        # (c): slots of every kind, evenly spread, within the bound
        for kind in (1, 2, 3):
            slots = np.argwhere(inp.face_kind == kind)
            for a, f in slots[:: max(1, len(slots) // MP_SLOTS)]:
                value, bound = kr.mp_face(inp, u, int(a), int(f))
                assert abs(host.face_int[a, f] - value) <= bound, (cycle, a, f)
                worst = max(worst, abs(host.face_int[a, f] - value) / bound)
        for a in range(0, inp.n_cells, max(1, inp.n_cells // MP_SLOTS)):
            value, bound = kr.mp_residual(inp, inp.dens, a)
            assert abs(host.residual_sq[a] - value) <= bound, (cycle, a)
        # marks against (c).  The float eta of a cell lies within 2^-20 relative of its 50-digit value (kelly_reference.mp_eta:
        # (2 dim + 3) 2^-24 plus face bounds of the order 2^-45), so a cell whose eta is further than 2^-18 relative from the
        # threshold has the same mark in both; every cell closer than that, and the maximum, is evaluated at 50 digits.
        res = inp.residual if inp.residual == 1 else 0
        eta = host.eta.astype(np.float64)
        top = int(np.argmax(eta))
        e_top, tol_top = kr.mp_eta(inp, u, inp.dens, res, top)
        thr, thr_tol = inp.fraction * e_top, inp.fraction * tol_top
        assert abs(host.threshold - thr) <= thr_tol
        near = np.nonzero(np.abs(eta - host.threshold) <= 2.0 ** -18 * host.threshold)[0]
        for a in near:
            e, tol = kr.mp_eta(inp, u, inp.dens, res, int(a))
            assert abs(e - thr) > tol + thr_tol, (cycle, a)  # no cell may be left out
            assert int(e >= thr) == host.mark[a], (cycle, a)
    print(f"{name} {rule}: worst face error / bound {worst:.3f}, slots by kind {seen}")
    assert np.all(seen > 0), seen
    p.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_two_gauss_points_integrate_the_squared_jump_exactly(dim):
    """ng = degree + 1 = 2: the quadrature sum of a squared bilinear jump equals measure / 36 c^T M c to the bound"""
    forest = kr.Forest(dim, 2, h0=0.75)
    inp = kr.inputs(forest, ng=2)
    u = kr.solution(inp, "smooth")
    fi = kr.face_integrals(inp, u)
    n = 0
    for a, f in np.argwhere(inp.face_kind == 1):
        d, side = f >> 1, f & 1
        b = inp.face_cell[a, f, 0]
        m, p = (a, b) if side else (b, a)
        jump = kr.corner_gradients(inp, u, np.array([p]), d)[0] - kr.corner_gradients(inp, u, np.array([m]), d)[0]
        exact = kr.closed_form(inp, jump, inp.face_measure_of_level[0])
        value, bound = kr.mp_face(inp, u, int(a), int(f))
        assert abs(value - exact) <= bound and abs(fi[a, f] - exact) <= 2 * bound and exact > 0
        n += 1
    assert n == (8 if dim == 2 else 24)
    one = kr.inputs(forest, ng=1)  # one point does not: the rule is pinned
    assert np.abs(kr.face_integrals(one, u) - fi).max() > 1e-6


def test_synthetic_face_tables():
    inp = kr.inputs(kr.Forest(2, 2).refine(0))
    assert inp.n_cells == 7 and list(np.bincount(inp.face_kind.ravel(), minlength=4)) == [10, 12, 2, 4]
    with pytest.raises(ValueError):
        kr.inputs(kr.Forest(2, 2).refine(0).refine(4))  # grandchildren beside a root cell
    assert kr.inputs(kr.centre_refined(2)).n_cells == 62 and kr.inputs(kr.uniform(3, 4).refine(21)).n_cells == 71


def test_key_defaults_to_the_host_loop(golden_dir):
    p = problem(golden_dir, "atom_n1_8.data", 1.0, 1, "Kelly + residual")
    p.run_cycle(0, on_device=False)
    p.finish_cycle_with(stand_in_solution(p))
    assert not p.estimated_on_device() and "Error estimator on device" not in p.log()
    q = problem(golden_dir, "atom_n1_8.data", 1.0, 1, "Kelly + residual", estimator_on_device=True)
    q.run_cycle(0, on_device=False)
    q.finish_cycle_with(stand_in_solution(q))
    assert not q.estimated_on_device() and q.log().count("Error estimator on device: not applicable") == 1
    assert kr.same_bits(exported(p), exported(q)) == []
    p.close()
    q.close()


def test_null_context_and_python_side_validation():
    L = capi().load()
    assert L.gmg_estimate_error(None, *([None] * 28)) == capi().ERR_INVALID
    ctx = capi().Context.view(C.c_void_p())
    inp = kr.inputs(kr.Forest(2, 2).refine(0))
    args = dict(dim=2, cell_dofs=inp.cell_dofs, cell_level=inp.cell_level, face_kind=inp.face_kind, face_cell=inp.face_cell,
                h_of_level=inp.h_of_level, face_measure_of_level=inp.face_measure_of_level, diameter_of_level=inp.diameter_of_level,
                gauss_x=inp.gauss_x, gauss_w=inp.gauss_w, u=None)
    for bad in (dict(dim=4), dict(cell_dofs=inp.cell_dofs[:, :3]), dict(face_kind=inp.face_kind[:-1]), dict(face_cell=inp.face_cell[:, :, :1]),
                dict(h_of_level=inp.h_of_level[:15]), dict(gauss_w=inp.gauss_w[:1]), dict(residual=1, weight=np.ones(4) / 4)):
        with pytest.raises(ValueError):
            ctx.estimate_error(**dict(args, **bad))
