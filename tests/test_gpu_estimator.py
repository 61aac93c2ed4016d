"""gmg_estimate_error on the MI355X (csrc/gmg_estimate.hpp) against the independent restatement of tests/kelly_reference.py
-- bit for bit against its numpy part, within the derived bound against its 50-digit part --, against the host loops of
the driver on the golden meshes, against the thresholds the reference printed, and whole adaptive runs with
"Error estimator on device" against the same runs without it."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import kelly_reference as kr
from conftest import rel_close
from gpu_util import capi, pkg
from test_gpu_system_matrix import END_TO_END

pytestmark = pytest.mark.gpu

FORESTS = {
    "single-2d": lambda: kr.Forest(2, 1),
    "single-3d": lambda: kr.Forest(3, 1),
    "2x2-one-refined-2d": lambda: kr.Forest(2, 2).refine(0),
    "3x3x3-centre": lambda: kr.centre_refined(1),
    "3x3x3-centre-twice": lambda: kr.centre_refined(2),
    "4x4x4": lambda: kr.uniform(3, 4),
    "4x4x4-one-refined": lambda: kr.uniform(3, 4).refine(21),
    "random-depth-3": lambda: kr.random_forest(),
}


@pytest.fixture()
def ctx():
    c = capi().Context(1)
    yield c
    c.close()


def run(ctx, inp, u, residual=0, dens=None, resident=False, **kw):
    v = ctx.vector(len(u), u)
    try:
        return ctx.estimate_error(inp.dim, inp.cell_dofs, inp.cell_level, inp.face_kind, inp.face_cell, inp.h_of_level,
                                  inp.face_measure_of_level, inp.diameter_of_level, inp.gauss_x, inp.gauss_w, v, residual=residual,
                                  weight=inp.weight if residual else None, jxw_of_level=inp.jxw_of_level if residual else None,
                                  dens=None if resident else dens, fraction=inp.fraction, **kw)
    finally:
        v.free()


def densities(inp, seed=3):
    return np.abs(np.random.default_rng(seed).standard_normal((inp.n_cells, inp.nq))) * 0.05


@pytest.mark.parametrize("name", list(FORESTS))
def test_abi_equals_the_numpy_restatement(ctx, name):
    forest = FORESTS[name]()
    cases = [("smooth", 2, 1, 2), ("constant", 2, 1, 2), ("linear", 2, 1, 2), ("smooth", 1, 0, 0), ("smooth", 3, 2, 1), ("smooth", 2, 1, 5)]
    kinds = np.zeros(4, dtype=np.int64)
    for what, ng, residual, nq1 in cases:
        inp = kr.inputs(forest, ng=ng, nq1=nq1)
        kinds += np.bincount(inp.face_kind.ravel(), minlength=4)
        u = kr.solution(inp, what)
        dens = densities(inp) if residual else None
        ref = kr.estimate(inp, u, dens=dens, residual=residual)
        for max_blocks in (0, 1, 3):
            ctx.set_option("estimate_max_blocks", max_blocks)
            dev = run(ctx, inp, u, residual=residual, dens=dens)
            assert kr.same_bits(dev, ref) == [], (what, ng, residual, nq1, max_blocks)
        if what == "constant" and residual == 1:
            dev0 = run(ctx, inp, u)  # no residual: every eta is 0 and every cell is marked
            assert not dev0.eta.any() and dev0.threshold == 0.0 and dev0.n_marked == inp.n_cells and dev0.mark.all()
        if what == "linear":
            assert np.all(dev.kelly_sq < 1e-24), dev.kelly_sq.max()  # the jumps cancel to rounding
    if name == "2x2-one-refined-2d":
        assert np.all(kinds > 0), kinds  # kinds 0-3 are all present


def test_densities_resident_on_the_device(ctx):
    """the densities gmg_charge_density(dens = NULL) left on the device, against the same values as a host array"""
    forest = kr.centre_refined(2)
    inp = kr.inputs(forest, ng=2, nq1=2)
    lv, lo, size, L = forest.boxes()
    cell_h = inp.h_of_level[lv]
    cell_lo = np.zeros((inp.n_cells, 3))
    cell_lo[:, :3] = lo * (forest.h0 / (1 << L))
    x1, _ = kr.gauss01(2)
    qp = np.array([[x1[q & 1], x1[(q >> 1) & 1], x1[q >> 2]] for q in range(8)])
    xyz, q = np.array([[1.4, 1.5, 1.6], [0.4, 2.2, 1.1]]), np.array([1.0, -1.0])
    u = kr.solution(inp, "smooth")
    ctx.charge_density(cell_lo, cell_h, np.floor(cell_lo), 1.0, xyz, q, 0.5, 10.0, False, qp, dens=None)
    dens = ctx.get_charge_density(inp.n_cells, 8)
    assert np.abs(dens).max() > 0
    for residual in (1, 2):
        ref = kr.estimate(inp, u, dens=dens, residual=residual)
        assert kr.same_bits(run(ctx, inp, u, residual=residual, resident=True), ref) == [], residual
        assert kr.same_bits(run(ctx, inp, u, residual=residual, dens=dens), ref) == [], residual
    bad = kr.inputs(kr.centre_refined(1), ng=2, nq1=2)  # another number of cells
    with pytest.raises(capi().GMGError) as e:
        run(ctx, bad, kr.solution(bad, "smooth"), residual=1, resident=True)
    assert e.value.code == capi().ERR_INVALID


@pytest.mark.parametrize("name", list(FORESTS))
def test_values_and_marks_against_50_digits(ctx, name):
    """face_int and residual_sq within the bound kelly_reference.py derives; marks equal to those of the 50-digit eta, where
    a cell may be left out only if its eta lies within the bound of the threshold -- and on these inputs none may"""
    inp = kr.inputs(FORESTS[name](), ng=2, nq1=2)
    u, dens = kr.solution(inp, "smooth"), densities(inp)
    dev = run(ctx, inp, u, residual=1, dens=dens)
    worst = 0.0
    for a in range(inp.n_cells):
        for f in range(2 * inp.dim):
            value, bound = kr.mp_face(inp, u, a, f)
            assert abs(dev.face_int[a, f] - value) <= bound, (a, f)
            worst = max(worst, abs(dev.face_int[a, f] - value) / bound if bound else 0.0)
        value, bound = kr.mp_residual(inp, dens, a)
        assert abs(dev.residual_sq[a] - value) <= bound, a
        worst = max(worst, abs(dev.residual_sq[a] - value) / bound)
    print(f"{name}: worst error / bound {worst:.3f}")
    eta = [kr.mp_eta(inp, u, dens, 1, a) for a in range(inp.n_cells)]
    top = max(range(inp.n_cells), key=lambda a: eta[a][0])
    thr, thr_tol = inp.fraction * eta[top][0], inp.fraction * eta[top][1]
    left_out = [a for a in range(inp.n_cells) if abs(eta[a][0] - thr) <= eta[a][1] + thr_tol and a != top]
    # (a single cell is its own maximum: it sits above the threshold 0.6 max by construction, nothing is near)
    assert left_out == [], left_out
    assert [int(e[0] >= thr) for e in eta] == list(dev.mark)
    assert abs(dev.threshold - thr) <= thr_tol


GOLDEN = [("atom_n1_8.data", 1.0, 3), ("atom_n3_216.data", 3.0, 2), ("atom_n5_1000.data", 5.0, 3)]


def golden_problem(golden_dir, name, right, cycles, rule, **kw):
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=2, problem="GaussianCharges", dim=3, bc="Exact", cycles=cycles,
                             r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR",
                             refinement_estimator=rule, **kw))
    p.read_lammps(os.path.join(golden_dir, name))
    return p


def exported(p):
    k, r, _, _ = p.estimator_components()
    return SimpleNamespace(face_int=p.face_integrals(), kelly_sq=k, residual_sq=r, eta=p.error_per_cell(), mark=p.marks(),
                           threshold=p.report()["refine_threshold"], n_marked=int(p.marks().sum()))


@pytest.mark.parametrize("rule", ["Kelly + residual", "Kelly"])
@pytest.mark.parametrize("name,right,cycles", GOLDEN, ids=[m[0] for m in GOLDEN])
def test_device_equals_host_on_golden_meshes(golden_dir, name, right, cycles, rule):
    p = golden_problem(golden_dir, name, right, cycles, rule, estimator_on_device=True)
    for cycle in range(cycles):
        copies = p.host_density_copies()  # (only the host re-run below of an earlier cycle has fetched densities)
        assert copies == (cycle if rule != "Kelly" else 0)
        p.run_cycle(cycle, on_device=True)
        assert p.estimated_on_device() and "not applicable" not in p.log()
        first = exported(p)
        inp = p.estimator_inputs()
        assert inp.residual == (1 if rule != "Kelly" else 0) and inp.dens_resident == (rule != "Kelly")
        assert p.host_density_copies() == copies  # the densities of "RHS on device" did not leave the device in this cycle
        p.estimate(on_device=True)
        dev = exported(p)
        assert p.estimated_on_device() and kr.same_bits(dev, first) == [] and p.host_density_copies() == copies
        # the independent restatement from the exported inputs (the resident densities fetched through the library, not the driver)
        u = p.vector("solution")
        dens = capi().Context.view(p.gmg_context()).get_charge_density(inp.n_cells, inp.nq) if inp.dens_resident else inp.dens
        assert kr.same_bits(dev, kr.estimate(inp, u, dens=dens)) == [], cycle
        p.estimate(on_device=False)
        host = exported(p)
        assert not p.estimated_on_device()
        assert kr.same_bits(dev, host) == [], cycle
        assert p.host_density_copies() == (cycle + 1 if rule != "Kelly" else 0)
        assert p.log().count("Threshold value for refinement") == 3 * (cycle + 1)
    assert (inp.face_kind == 2).any() and (inp.face_kind == 3).any()
    p.close()


def test_reference_thresholds_and_refinement(golden, golden_dir):
    """the six cycles of the reference's regression test with the estimator on the device: the printed thresholds to 11
    digits, the iteration counts, and the cells and DoFs of every following cycle -- the marks drove the same refinement"""
    S = pkg().step50
    G = golden["tests/gaussian-charges.mpirun=1"]["runs"][0]["cycles"]
    p = S.Problem(S.prm_text(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Exact", cycles=6, r_c=0.5,
                             cutoff=3.5, rhs_optimization=True, quad_rhs=4, global_refinement=0, smoother="SSOR", partition_level0="always",
                             estimator_on_device=True))
    p.read_lammps(os.path.join(golden_dir, "atom_n1_2.data"))
    reps = []
    for cycle in range(6):
        reps.append(p.run_cycle(cycle, on_device=True))
        assert p.estimated_on_device()
    assert p.host_density_copies() == 0
    assert [r["cg_iterations"] for r in reps] == [1, 6, 7, 6, 7, 7]
    for r, g in zip(reps, G):
        assert rel_close(r["refine_threshold"], g["refine_threshold"], 11), (r["cycle"], r["refine_threshold"], g["refine_threshold"])
        assert r["active_cells"] == g["active_cells"] and r["dofs"] == g["dofs"] and r["dofs_by_level"] == g["dofs_by_level"]
    p.close()


@pytest.mark.parametrize("name,right,cycles", END_TO_END, ids=[m[0] for m in END_TO_END])
def test_adaptive_run_is_unchanged(golden_dir, name, right, cycles):
    S = pkg().step50
    runs = {}
    for key in (False, True):
        p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous",
                                 cycles=cycles, r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR",
                                 refinement_estimator="Kelly", estimator_on_device=key))
        p.read_lammps(os.path.join(golden_dir, name))
        out = []
        for cycle in range(cycles):
            rep = p.run_cycle(cycle, on_device=True)
            assert p.estimated_on_device() == key
            out.append((rep, p.refine_flags(), p.error_per_cell()))
        runs[key] = out
        p.close()
    for cycle, ((r0, f0, e0), (r1, f1, e1)) in enumerate(zip(runs[False], runs[True])):
        for k in r0:
            if k == "energy_norm_error":  # the host sums it with an OpenMP reduction over dynamic chunks: its last bits vary from run to run
                assert abs(r0[k] - r1[k]) <= 1e-12 * abs(r0[k]), (cycle, k, r0[k], r1[k])
            elif k not in ("solve_seconds", "build_matrices_ms"):  # (times)
                assert r0[k] == r1[k], (cycle, k, r0[k], r1[k])
        assert np.array_equal(f0, f1) and e0.tobytes() == e1.tobytes(), cycle


def test_invalid_arguments_are_refused_and_the_context_survives(ctx):
    good = kr.inputs(kr.Forest(2, 2).refine(0), ng=2, nq1=2)
    u, dens = kr.solution(good, "smooth"), densities(good)
    ref = kr.estimate(good, u, dens=dens, residual=1)

    def changed(**kw):
        d = dict(vars(good))
        d.update(kw)
        return SimpleNamespace(**d)

    def with_entry(a, idx, v):
        a = np.array(a)
        a[idx] = v
        return a

    k1 = tuple(np.argwhere(good.face_kind == 1)[0])
    k2 = tuple(np.argwhere(good.face_kind == 2)[0])
    k3 = tuple(np.argwhere(good.face_kind == 3)[0])
    bad = {
        "dim": (changed(dim=4), {}),
        "level": (changed(cell_level=with_entry(good.cell_level, 0, 16)), {}),
        "dof below": (changed(cell_dofs=with_entry(good.cell_dofs, (1, 1), -1)), {}),
        "dof above": (changed(cell_dofs=with_entry(good.cell_dofs, (1, 1), good.n_u)), {}),
        "kind": (changed(face_kind=with_entry(good.face_kind, k1, 4)), {}),
        "face_cell below": (changed(face_cell=with_entry(good.face_cell, k1 + (0,), -1)), {}),
        "face_cell above": (changed(face_cell=with_entry(good.face_cell, k2 + (1,), good.n_cells)), {}),
        "kind 1 level": (changed(face_kind=with_entry(good.face_kind, k3, 1)), {}),
        "kind 2 level": (changed(face_kind=with_entry(good.face_kind, k1, 2)), {}),
        "kind 3 level": (changed(face_kind=with_entry(good.face_kind, k1, 3)), {}),
        "quadrant": (changed(face_cell=with_entry(good.face_cell, k3 + (1,), 2)), {}),
        "ng 0": (changed(gauss_x=np.zeros(0), gauss_w=np.zeros(0)), {}),
        "ng 9": (changed(gauss_x=np.full(9, 0.5), gauss_w=np.full(9, 1 / 9)), {}),
        "nq 513": (changed(weight=np.full(513, 1 / 513)), dict(dens=np.zeros((good.n_cells, 513)))),
        "fraction < 0": (changed(fraction=-0.1), {}),
        "fraction nan": (changed(fraction=float("nan")), {}),
        "fraction inf": (changed(fraction=float("inf")), {}),
        "no device densities": (good, dict(resident=True)),
        "null": (changed(face_kind=np.zeros(0, dtype=np.uint8)), {}),
    }
    for what, (inp, kw) in bad.items():
        with pytest.raises(capi().GMGError) as e:
            run(ctx, inp, u, **dict(dict(residual=1, dens=dens, validate=False), **kw))
        assert e.value.code == capi().ERR_INVALID and "gmg_estimate_error" in str(e.value), what
        assert kr.same_bits(run(ctx, good, u, residual=1, dens=dens), ref) == [], what  # the context works as before
    # nq 0 with a residual
    with pytest.raises(capi().GMGError) as e:
        run(ctx, changed(weight=np.zeros(0)), u, residual=1, dens=np.zeros((good.n_cells, 0)), validate=False)
    assert e.value.code == capi().ERR_INVALID
    L = capi().load()
    assert L.gmg_estimate_error(None, *([None] * 28)) == capi().ERR_INVALID


def test_zero_cells_and_reset(ctx):
    some = kr.inputs(kr.Forest(3, 1), ng=2)
    empty = SimpleNamespace(**dict(vars(some), cell_dofs=np.zeros((0, 8), dtype=np.int32), cell_level=np.zeros(0, dtype=np.uint8),
                                   face_kind=np.zeros((0, 6), dtype=np.uint8), face_cell=np.zeros((0, 6, 4), dtype=np.int32), n_cells=0))
    out = run(ctx, empty, np.zeros(4))
    assert out.threshold == 0.0 and out.n_marked == 0 and len(out.eta) == 0
    inp = kr.inputs(kr.centre_refined(1), ng=2)
    u = kr.solution(inp, "smooth")
    ref = kr.estimate(inp, u)
    assert kr.same_bits(run(ctx, inp, u), ref) == []
    assert ctx.L.gmg_reset(ctx.h, C.c_int(1)) == capi().OK
    assert kr.same_bits(run(ctx, inp, u), ref) == []


def test_driver_falls_back_to_the_host_on_a_communicator(golden_dir):
    p = golden_problem(golden_dir, "atom_n1_8.data", 1.0, 2, "Kelly + residual", estimator_on_device=True)
    p.set_communicator(0, 1, capi().Context.unique_id())
    for cycle in range(2):
        p.run_cycle(cycle, on_device=True)
        assert not p.estimated_on_device()
    assert p.log().count("Error estimator on device: not applicable (the run is distributed)") == 1
    p.close()


def test_no_leak_across_calls():
    """free device memory after six rounds of a refused and an accepted call, in the manner of test_gpu_lifecycle.py"""
    from test_gpu_lifecycle import free_after_rounds

    inp = kr.inputs(kr.random_forest(), ng=2, nq1=2)
    u, dens = kr.solution(inp, "smooth"), densities(inp)
    bad_kind = np.array(inp.face_kind)
    bad_kind[0, 0] = 9

    def one_round():
        c = capi().Context(1)
        try:
            with pytest.raises(capi().GMGError):
                run(c, SimpleNamespace(**dict(vars(inp), face_kind=bad_kind)), u)
            with pytest.raises(capi().GMGError):
                run(c, inp, u, residual=1, resident=True)
            run(c, inp, u, residual=1, dens=dens)
        finally:
            c.close()

    free = free_after_rounds(one_round)
    assert free[-1] == free[0], free
