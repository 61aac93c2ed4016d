"""The Lanczos bound of lambda_max(D^-1 A) and the fourth-kind Chebyshev smoother on the device (gmg_estimate_lmax,
gmg_set_chebyshev, gmg_get_chebyshev; csrc/gmg_lanczos.hpp, cheb_apply in csrc/gmg_coulomb.hip) through capi.Context against
tests/cheb4_reference.py.  Tolerances follow section 16: TOL_FACTOR x the spread of the reference's two
tiers on the quantity compared x its norm, plus the coarse allowance where a level-0 solve is part of the result.
tests/test_cheb4_reference_cpu.py proves that every mutation of the derivation is 1000 tolerances or more away.  Each test
prints its worst error / tolerance ("[cheb4-gpu]", run with -s)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import cg_reference as CG
import cheb4_reference as C4
import mg_cases as K
import mg_reference as R
import test_gpu_mg_reference as G
from gpu_util import capi, pkg
from oracle import gmg_oracle as go

pytestmark = pytest.mark.gpu

TAU = 1e-10
STEPS = 10
DEGREES = (1, 2, 3, 4, 5)
USER_LMAX = 1.7


def set4(c, cfg):
    """the smoother of a Config4 (fourth kind) or of a mg_reference.Config (first kind, Gershgorin)"""
    A = capi()
    c.set_smoother(A.CHEBYSHEV, cfg.omega, cfg.steps, cheb_degree=cfg.degree, cheb_ratio=cfg.ratio, cheb_lmax=cfg.lmax)
    if cfg.kind == C4.CHEB4:
        c.set_chebyshev(A.CHEB_FOURTH_KIND, cfg.source, cfg.lanczos_steps, cfg.safety)
    else:
        c.set_chebyshev(A.CHEB_FIRST_KIND, A.CHEB_LMAX_GERSHGORIN)


def check_estimate(e, ref, what):
    """a device estimate (capi.Context.estimate_lmax) against cheb4_reference.lanczos_reference -> worst error / tolerance"""
    m = ref.steps_run
    assert e["steps_run"] == m, (what, e["steps_run"], m)
    assert not e["alpha"][m:].any() and not e["beta"][m:].any(), what
    ea, eb = float(np.linalg.norm(e["alpha"][:m] - ref.alpha)), float(np.linalg.norm(e["beta"][:m] - ref.beta))
    er = abs(e["ritz"] - ref.ritz)
    print(f"\n[cheb4-gpu] estimate {what}: error / tolerance alpha {ea / ref.tol_alpha:.3f} beta {eb / ref.tol_beta:.3f} ritz {er / ref.tol_ritz:.3f}; "
          f"ritz {e['ritz']:.12f}, steps {m}")
    assert ea <= ref.tol_alpha and eb <= ref.tol_beta and er <= ref.tol_ritz, (what, ea, ref.tol_alpha, eb, ref.tol_beta, er, ref.tol_ritz)
    return max(ea / ref.tol_alpha, eb / ref.tol_beta, er / ref.tol_ritz)


@pytest.fixture(scope="module")
def ctx():
    made = {}

    def get(name):
        if name not in made:
            made[name] = G.context(name)
        return made[name]

    yield get
    for c in made.values():
        c.close()


# ------------------------------------------------------------------------------------------------ the estimate

@pytest.mark.parametrize("name,level", K.SMOOTH_LEVELS)
def test_estimate_accuracy(ctx, name, level):
    """alpha, beta and ritz within the tolerance made of the tiers' spread of each; steps_run; a second call and a call with the
    grids capped at one and at three workgroups give the same bits"""
    c = ctx(name)
    ref = C4.lanczos_reference(name, level, STEPS)
    before = c.get_chebyshev(level)
    e = c.estimate_lmax(level, STEPS)
    check_estimate(e, ref, f"{name} level {level}")
    for cap in (0, 1, 3):
        c.set_option("lanczos_max_blocks", cap)
        e2 = c.estimate_lmax(level, STEPS)
        assert e2["steps_run"] == e["steps_run"] and e2["ritz"] == e["ritz"], cap
        assert np.array_equal(e2["alpha"], e["alpha"]) and np.array_equal(e2["beta"], e["beta"]), cap
    c.set_option("lanczos_max_blocks", 0)
    short = c.estimate_lmax(level, 3, coefficients=False)    # (NULL arrays; fewer steps: a prefix of the same recurrence)
    e3 = c.estimate_lmax(level, 3)
    assert short["ritz"] == e3["ritz"] and np.array_equal(e3["alpha"], e["alpha"][:3]) and np.array_equal(e3["beta"], e["beta"][:3])
    assert c.get_chebyshev(level) == before                  # (the estimate on request changes nothing the smoother uses)


def test_estimate_level0_lattice():
    """level 0 formed on the device (gmg_set_level_matrix_lattice: the plane-by-plane lattice kernel forms A p)"""
    shape, Ke, _ = K.level0_lattice("A3")
    c = G.context("A3", lattice=(shape, Ke))
    assert int(c.stats().spmv0_layout) & 64
    check_estimate(c.estimate_lmax(0, STEPS), C4.lanczos_reference("A3", 0, STEPS), "A3 level 0, lattice operator")
    c.close()


def layout_run(switch):
    """LAT under one layout switch (None: the default layouts), a context of its own: the estimate on both levels and the whole
    sweep of cheb4_configs() on level 1, apply and smooth, each checked against the reference -> every result, by key"""
    c = G.context(K.LAT, options=() if switch is None else ((switch, 1),))
    what = switch or "default"
    got = {}
    for level in (1, 0):
        e = c.estimate_lmax(level, STEPS)
        check_estimate(e, C4.lanczos_reference(K.LAT, level, STEPS), f"LAT level {level} {what}")
        got["e", level] = np.concatenate([e["alpha"], e["beta"], [e["ritz"]]])
    u0, rhs = K.smoother_vectors(K.LAT, 1)
    worst = 0.0
    for cfg in cheb4_configs():
        set4(c, cfg)
        for from_zero in (True, False):
            ref = C4.smoother_reference(K.LAT, 1, cfg, from_zero)
            out = G.smooth(c, 1, u0, rhs, from_zero)
            err = float(np.linalg.norm(out - ref.ref))
            worst = max(worst, err / ref.tol)
            assert err <= ref.tol, (what, cfg.label(), from_zero, err, ref.tol)
            got["s", cfg, from_zero] = out
    c.close()
    print(f"\n[cheb4-gpu] layouts LAT {what}: {len(got) - 2} smoother results, error / tolerance max {worst:.3f}")
    return got


@pytest.fixture(scope="module")
def layout_default():
    return layout_run(None)


@pytest.mark.parametrize("switch", K.LAYOUT_SWITCHES)
def test_layouts(layout_default, switch):
    """LAT (level 1 in SELL-64 with every layout bit, level 0 on CSR row windows) under each switch that changes the kernel
    behind the level's product and its Chebyshev epilogue (row windows, SELL-64 with and without patterns, value codes and
    16-bit columns, the pattern-run kernel with and without row classes, the lattice kernel): the estimate on both levels and
    the fourth-kind smoother steps on level 1 -- degrees 1 to 5, 0 to 3 steps, apply and smooth, under the Gershgorin bound,
    the Lanczos bound and a user bound -- are within tolerance of the reference, by default (the fixture) and under the
    switch; a row is summed in its stored order in every layout, so the switch also gives the default's bits"""
    got = layout_run(switch)
    assert got.keys() == layout_default.keys()
    differ = [k[:1] + tuple(str(x) for x in k[1:]) for k, v in got.items() if not np.array_equal(v, layout_default[k])]
    assert not differ, (switch, differ)


def one_row():
    return SimpleNamespace(n_rows=1, n_cols=1, nnz=1, rowptr=np.array([0, 1], dtype=np.int64), col=np.array([0], dtype=np.int32), val=np.array([2.5]))


def test_corner_cases(ctx):
    """a one-row level and hier3 level 1 (27 boundary rows): D^-1 A = I, the recurrence ends after one step with ritz 1 (alpha 1
    up to the rounding of (r / a) a, beta below the breakdown threshold); the smoother then uses min(1.2, Gershgorin = 1) = 1.
    A level whose rows hold their own diagonal has a Gershgorin bound of 1 or more.  A bound of 0 needs a level without rows
    or of empty rows; the estimate then runs no step and the level keeps Gershgorin, as the definition says.  So the branch
    "safety x ritz where there is no Gershgorin bound" of the bound in use cannot be reached through the ABI and has no case
    here; the reference carries it (cheb4_reference.bound)"""
    A = capi()
    c = A.Context(1)
    c.set_level_matrix(0, one_row())
    e = c.estimate_lmax(0, STEPS)
    assert e["steps_run"] == 1 and abs(e["ritz"] - 1.0) <= 8 * R.U and abs(e["alpha"][0] - 1.0) <= 8 * R.U and 0.0 <= e["beta"][0] <= 2.0 ** -100
    c.close()
    c = ctx("hier3")
    check_estimate(c.estimate_lmax(1, STEPS), C4.lanczos_reference("hier3", 1, STEPS), "hier3 level 1")
    e = c.estimate_lmax(1, STEPS)
    assert e["steps_run"] == 1 and abs(e["ritz"] - 1.0) <= 8 * R.U
    cfg = C4.Config4(degree=3, steps=2, source=C4.LANCZOS)
    set4(c, cfg)
    u0, rhs = K.smoother_vectors("hier3", 1)
    ref = C4.smoother_reference("hier3", 1, cfg, True)
    assert float(np.linalg.norm(G.smooth(c, 1, u0, rhs, True) - ref.ref)) <= ref.tol
    info = c.get_chebyshev(1)
    assert info["steps_run"] == 1 and info["gershgorin"] == 1.0 and info["lmax"] == 1.0
    set4(c, R.Config(kind=R.CHEBYSHEV))


def refused(call, code):
    with pytest.raises(capi().GMGError) as e:
        call()
    assert e.value.code == code, (e.value.code, code)


def test_refusals(ctx):
    A = capi()
    c = ctx("SYN")
    before = c.get_chebyshev(1)
    for args in ((2, 0, 0, 0.0), (-1, 0, 0, 0.0), (0, 2, 0, 0.0), (0, -1, 0, 0.0), (1, 1, 65, 0.0), (1, 1, -1, 0.0), (1, 1, 0, 0.5), (1, 1, 0, -1.0),
                 (1, 1, 0, float("nan")), (1, 1, 0, float("inf"))):
        refused(lambda: c.set_chebyshev(*args), A.ERR_INVALID)
    for key, value in (("cheb_polynomial", 2), ("cheb_polynomial", 0.5), ("cheb_polynomial", 1e10), ("cheb_lmax_source", float("nan")), ("cheb_lmax_source", 3), ("cheb_lanczos_steps", 0), ("cheb_lanczos_steps", 65),
                       ("cheb_safety", 0.9), ("cheb_degree", -1), ("cheb_degree", 1.5), ("lanczos_max_blocks", -1)):
        refused(lambda: c.set_option(key, value), A.ERR_INVALID)
    assert c.get_chebyshev(1) == before                      # (a refused call changes nothing)
    for level, steps in ((-1, 10), (2, 10), (1, 0), (1, 65), (1, -3)):
        refused(lambda: c.estimate_lmax(level, steps), A.ERR_INVALID)
    import ctypes

    run = ctypes.c_int(0)
    assert c.L.gmg_estimate_lmax(c.h, ctypes.c_int(1), ctypes.c_int(10), None, None, None, ctypes.byref(run)) == A.ERR_INVALID
    f = A.Context(2)                                         # a level that has not been set
    refused(lambda: f.estimate_lmax(1, 10), A.ERR_INVALID)
    assert f.get_chebyshev(1) == dict(zip(A.CHEBYSHEV_KEYS, (0, 0, 10, 0, 0, 0, 1.2, 0)))
    f.close()
    m = K.hierarchy("SYN")[0].level_matrices[0]              # a row-partitioned level 0 (one rank holds all of it: still refused)
    p = A.Context(1)
    p.comm_init(0, 1, A.Context.unique_id())
    p.set_global_sizes(m.n_rows, m.n_rows)
    p.set_level_matrix(0, m)
    refused(lambda: p.estimate_lmax(0, 10), A.ERR_UNSUPPORTED)
    p.close()


# ------------------------------------------------------------------------------------------------ smoother steps

def cheb4_configs():
    out = []
    for s in (0, 1, 2, 3):
        for k in DEGREES:
            out += [C4.Config4(degree=k, steps=s), C4.Config4(degree=k, steps=s, source=C4.LANCZOS), C4.Config4(degree=k, steps=s, lmax=USER_LMAX)]
    return out


@pytest.mark.parametrize("name,level", K.SMOOTH_LEVELS)
def test_smoother_step(ctx, name, level):
    """the fourth kind with degrees 1 to 5 and 0 to 3 steps, apply and smooth, under the Gershgorin bound, the Lanczos bound and
    a user bound; and the first kind under the Lanczos bound (the reference: mg_reference's first-kind operator given the
    reference's Lanczos bound as its lmax)"""
    A = capi()
    c = ctx(name)
    u0, rhs = K.smoother_vectors(name, level)
    worst = {}
    for cfg in cheb4_configs():
        set4(c, cfg)
        for from_zero in (True, False):
            ref = C4.smoother_reference(name, level, cfg, from_zero)
            err = float(np.linalg.norm(G.smooth(c, level, u0, rhs, from_zero) - ref.ref))
            key = "user" if cfg.lmax > 0 else ("lanczos" if cfg.source == C4.LANCZOS else "gershgorin")
            worst[key] = max(worst.get(key, 0.0), err / ref.tol)
            assert err <= ref.tol, (cfg.label(), from_zero, err, ref.tol, ref.S)
    lam = C4.hierarchy4(name).levels("ld")[level].lam(C4.Config4(source=C4.LANCZOS))
    first = R.Config(kind=R.CHEBYSHEV, steps=2, degree=3, lmax=lam)
    c.set_smoother(A.CHEBYSHEV, first.omega, first.steps, cheb_degree=3, cheb_ratio=first.ratio, cheb_lmax=0.0)
    c.set_chebyshev(A.CHEB_FIRST_KIND, A.CHEB_LMAX_LANCZOS)
    # both tiers of this reference are given ONE lmax, so their spread holds nothing of the bound's own rounding: the device's
    # bound is within 1.2 tol_ritz of it (asserted below), and the reference's own change under that shift is added
    dl = 1.2 * C4.lanczos_reference(name, level, STEPS).tol_ritz
    H = K.hierarchy(name)[1]
    for from_zero in (True, False):
        ref = K.smoother_reference(name, level, first, from_zero)
        shift = float(np.linalg.norm(H.smooth("f64", R.Config(kind=R.CHEBYSHEV, steps=2, degree=3, lmax=lam + dl), level, u0, rhs, from_zero)
                                     - H.smooth("f64", first, level, u0, rhs, from_zero)))
        err = float(np.linalg.norm(G.smooth(c, level, u0, rhs, from_zero) - ref.ref))
        worst["first kind, lanczos"] = max(worst.get("first kind, lanczos", 0.0), err / (ref.tol + shift))
        assert err <= ref.tol + shift, ("first kind, lanczos", from_zero, err, ref.tol, shift)
    info = c.get_chebyshev(level)
    assert info["polynomial"] == 0 and info["lmax_source"] == 1 and abs(info["lmax"] - lam) <= C4.lanczos_reference(name, level, STEPS).tol_ritz * 1.2
    set4(c, R.Config(kind=R.CHEBYSHEV))
    print(f"\n[cheb4-gpu] smoother_step {name} level {level}: error / tolerance max " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_first_kind_unchanged():
    """first kind and Gershgorin after gmg_set_chebyshev(ctx, 0, 0, 0, 0), and after a detour through the fourth kind and the
    Lanczos bound: the bits of a context that never made the call -- smoother steps and a V-cycle"""
    A = capi()
    name = "A3"
    src, labels, dst0 = K.vcycle_sources(name)
    cfgs = [R.Config(kind=R.CHEBYSHEV, steps=2, degree=3), R.Config(kind=R.CHEBYSHEV, steps=1, degree=2, ratio=4.0), R.Config(kind=R.CHEBYSHEV, steps=3, degree=4, lmax=1.7)]

    def run(c):
        out = []
        for cfg in cfgs:
            G.set_smoother(c, cfg)
            for level in (1, 2):
                u0, rhs = K.smoother_vectors(name, level)
                out += [G.smooth(c, level, u0, rhs, fz) for fz in (True, False)]
            out.append(G.precondition(c, src[:, 0], dst0))
        return out

    plain = G.context(name)
    base = run(plain)
    plain.close()
    c = G.context(name)
    c.set_chebyshev(0, 0, 0, 0.0)
    again = run(c)
    set4(c, C4.Config4(degree=3, steps=2, source=C4.LANCZOS))
    G.precondition(c, src[:, 0], dst0)
    c.set_chebyshev(A.CHEB_FIRST_KIND, A.CHEB_LMAX_GERSHGORIN)
    back = run(c)
    c.close()
    assert all(np.array_equal(a, b) for a, b in zip(base, again)) and all(np.array_equal(a, b) for a, b in zip(base, back))


# ------------------------------------------------------------------------------------------------ V-cycle and solve

VCYCLE4 = [C4.Config4(degree=3, steps=s, source=C4.LANCZOS) for s in (1, 2)]


@pytest.mark.parametrize("name", ["A3", "B3", "SYN"])
def test_precondition(name):
    """gmg_precondition with the fourth kind under the Lanczos bound, degree 3, 1 and 2 steps, against mg_reference's V-cycle
    with the fourth-kind operator put in (cheb4_reference.Hierarchy4), all sources of mg_cases.vcycle_sources"""
    H = C4.hierarchy4(name)
    zr = K.zero_rows(name)
    worst = 0.0
    for cfg in VCYCLE4:
        c = G.context(name)   # a context of its own: every level forms its bound inside the first V-cycle
        c.set_coarse(TAU, 1000)
        set4(c, cfg)
        assert all(c.get_chebyshev(l)["steps_run"] == 0 for l in range(1, H.n_levels))
        ref = C4.vcycle_reference(name, cfg)
        got = G.run_sources(c, name)
        for l in range(1, H.n_levels):
            info, lref = c.get_chebyshev(l), C4.lanczos_reference(name, l, STEPS)
            assert info["steps_run"] == lref.steps_run and abs(info["ritz"] - lref.ritz) <= lref.tol_ritz, (l, info)
        c.close()
        tol = ref.tol + H.cg_allowance(cfg, TAU)
        err = R.norm2(got - ref.ref)
        assert (err <= tol).all(), (cfg.label(), err, tol, ref.S)
        assert not got[zr].any(), cfg.label()
        worst = max(worst, float(np.max(err / tol)))
    print(f"\n[cheb4-gpu] precondition {name}: error / tolerance max {worst:.3f}")


@pytest.mark.parametrize("name", ["hier3", "A3", "B3"])
def test_cg_solve(ctx, name):
    """gmg_cg_solve with that preconditioner: the iteration count of cg_reference.cg with the reference's V-cycle as precond, at a
    tolerance cg_reference.target_tol accepts (every earlier residual 1.05 tol or more, the last tol / 1.05 or less), and the true
    residual, recomputed here, is below the tolerance"""
    h = K.hierarchy(name)[0]
    H = C4.hierarchy4(name)
    cfg = VCYCLE4[1]
    m, b = h.system_matrix, np.asarray(h.system_rhs, dtype=np.float64)

    def precond(_m, _tier):
        return lambda g: H.precondition("f64", cfg, np.asarray(g, dtype=np.float64))

    hist = CG.cg(m, b, 0.0, 16, precond=precond, keep_steps=False).history
    tol = None
    for k in range(3, 14):
        if hist[k] > 1e-6 * hist[0]:   # (a stop that means something: six digits; the residuals of the recurrence go on falling below
            continue                   # what a true residual can reach, so the first such k is taken, not a late one)
        try:
            tol = CG.target_tol(hist, k)
            break
        except ValueError:
            continue
    assert tol is not None, hist
    ref = CG.cg(m, b, tol, 500, precond=precond, keep_steps=False)
    assert ref.status == CG.OK and ref.iterations == k
    c = ctx(name)
    c.set_coarse(TAU, 1000)
    set4(c, cfg)
    n = m.n_rows
    vb, vx = c.vector(n, b), c.vector(n)
    r = c.cg_solve(vx, vb, rel_tol=tol / float(np.linalg.norm(b)), max_it=500)
    x = vx.download()
    vb.free()
    vx.free()
    set4(c, R.Config(kind=R.CHEBYSHEV))
    true_res = float(np.linalg.norm(b - go.spmv(m, x)))
    print(f"\n[cheb4-gpu] cg_solve {name}: {r['iterations']} iterations (reference {ref.iterations}), tolerance {tol:.3e}, true residual {true_res:.3e}, "
          f"|x - ref| / max|ref| {np.abs(x - ref.x).max() / np.abs(ref.x).max():.2e}")
    assert r["status"] == 0 and r["iterations"] == ref.iterations
    assert true_res <= tol


# ------------------------------------------------------------------------------------------------ lifetime

def lam_of(name, level, safety=1.2, steps=STEPS):
    ref = C4.lanczos_reference(name, level, steps)
    return min(safety * ref.ritz, ref.gershgorin), ref


def test_lifetime(capfd):
    """gmg_get_chebyshev before and after the first use; a level matrix replaced in place (SYN's A_1 by SYN-A1's, same pattern)
    gives a new estimate and the smoother follows it; a change of the steps or of the safety factor drops the estimate;
    gmg_reset; option debug_upload prints one line per estimate"""
    A = capi()
    h, ha = K.hierarchy("SYN")[0], K.hierarchy("SYN-A1")[0]
    cfg = C4.Config4(degree=3, steps=2, source=C4.LANCZOS)
    u0, rhs = K.smoother_vectors("SYN", 1)

    def check_smooth(c, name):
        for fz in (True, False):
            ref = C4.smoother_reference(name, 1, cfg, fz)
            err = float(np.linalg.norm(G.smooth(c, 1, u0, rhs, fz) - ref.ref))
            assert err <= ref.tol, (name, fz, err, ref.tol)

    c = G.context("SYN", options=(("debug_upload", 1),))
    set4(c, cfg)
    lam, ref = lam_of("SYN", 1)
    info = c.get_chebyshev(1)
    assert (info["polynomial"], info["lmax_source"], info["lanczos_steps"], info["steps_run"], info["ritz"], info["safety"], info["lmax"]) == (1, 1, 10, 0, 0, 1.2, 0)
    assert abs(info["gershgorin"] - ref.gershgorin) <= 8 * R.U * ref.gershgorin
    capfd.readouterr()
    check_smooth(c, "SYN")
    assert capfd.readouterr().err.count("[gmg] level 1 Chebyshev bound") == 1      # (the second call used the cached bound)
    info = c.get_chebyshev(1)
    assert info["steps_run"] == ref.steps_run and abs(info["ritz"] - ref.ritz) <= ref.tol_ritz and abs(info["lmax"] - lam) <= 1.2 * ref.tol_ritz
    # the matrix replaced in place
    lam_a, ref_a = lam_of("SYN-A1", 1)
    assert abs(ref_a.ritz - ref.ritz) >= 1000 * ref.tol_ritz                       # (the twin's bound is another one)
    c.set_level_matrix(1, ha.level_matrices[1])
    info = c.get_chebyshev(1)
    assert info["steps_run"] == 0 and info["ritz"] == 0 and info["lmax"] == 0
    check_smooth(c, "SYN-A1")
    info = c.get_chebyshev(1)
    assert abs(info["ritz"] - ref_a.ritz) <= ref_a.tol_ritz and abs(info["lmax"] - lam_a) <= 1.2 * ref_a.tol_ritz
    c.set_level_matrix(1, h.level_matrices[1])
    check_smooth(c, "SYN")
    # steps and safety
    c.set_chebyshev(A.CHEB_FOURTH_KIND, A.CHEB_LMAX_LANCZOS, 6, 0.0)
    assert c.get_chebyshev(1)["steps_run"] == 0 and c.get_chebyshev(1)["lanczos_steps"] == 6
    G.smooth(c, 1, u0, rhs, True)
    ref6 = C4.lanczos_reference("SYN", 1, 6)
    info = c.get_chebyshev(1)
    assert info["steps_run"] == 6 and abs(info["ritz"] - ref6.ritz) <= ref6.tol_ritz
    c.set_chebyshev(A.CHEB_FOURTH_KIND, A.CHEB_LMAX_LANCZOS, 0, 1.01)
    assert c.get_chebyshev(1)["steps_run"] == 0 and c.get_chebyshev(1)["safety"] == 1.01 and c.get_chebyshev(1)["lanczos_steps"] == 6
    G.smooth(c, 1, u0, rhs, True)
    info = c.get_chebyshev(1)
    assert abs(info["lmax"] - min(1.01 * ref6.ritz, ref6.gershgorin)) <= 1.2 * ref6.tol_ritz
    c.set_option("cheb_safety", 1.2)
    c.set_option("cheb_lanczos_steps", 10)
    assert c.get_chebyshev(1)["steps_run"] == 0
    # a user bound wins and needs no estimate
    c.set_smoother(A.CHEBYSHEV, 0.5, 2, cheb_degree=3, cheb_lmax=USER_LMAX)
    G.smooth(c, 1, u0, rhs, True)
    info = c.get_chebyshev(1)
    assert info["lmax"] == USER_LMAX and info["steps_run"] == 0
    # option cheb_degree overrides the degree of gmg_set_smoother
    set4(c, C4.Config4(degree=2, steps=2))
    c.set_option("cheb_degree", 4)
    ref4 = C4.smoother_reference("SYN", 1, C4.Config4(degree=4, steps=2), True)
    assert float(np.linalg.norm(G.smooth(c, 1, u0, rhs, True) - ref4.ref)) <= ref4.tol
    c.set_option("cheb_degree", 0)
    ref2 = C4.smoother_reference("SYN", 1, C4.Config4(degree=2, steps=2), True)
    assert float(np.linalg.norm(G.smooth(c, 1, u0, rhs, True) - ref2.ref)) <= ref2.tol
    # gmg_reset: nothing of the levels survives, the settings do
    set4(c, cfg)
    G.smooth(c, 1, u0, rhs, True)
    c.reset(2)
    info = c.get_chebyshev(1)
    assert (info["polynomial"], info["lmax_source"], info["steps_run"], info["gershgorin"], info["ritz"], info["lmax"]) == (1, 1, 0, 0, 0, 0)
    G.load(c, ha)
    check_smooth(c, "SYN-A1")
    c.close()


def test_defaults(ctx):
    """a context nobody told anything: first kind, Gershgorin, 10 steps, 1.2, lambda in use = the Gershgorin bound"""
    A = capi()
    c = A.Context(2)
    G.load(c, K.hierarchy("SYN")[0])
    g = C4.hierarchy4("SYN").levels("f64")[1].gershgorin
    info = c.get_chebyshev(1)
    assert (info["polynomial"], info["lmax_source"], info["lanczos_steps"], info["steps_run"], info["ritz"], info["safety"]) == (0, 0, 10, 0, 0, 1.2)
    assert abs(info["gershgorin"] - g) <= 8 * R.U * g and info["lmax"] == info["gershgorin"]
    c.close()


def test_no_leak():
    """free device memory over six rounds of create / load / estimate / smooth with the Lanczos bound / replace / reset / destroy,
    as tests/test_gpu_lifecycle.py does it: the first round absorbs what the runtime allocates once"""
    import torch

    h, ha = K.hierarchy("SYN")[0], K.hierarchy("SYN-A1")[0]
    u0, rhs = K.smoother_vectors("SYN", 1)
    cfg = C4.Config4(degree=3, steps=2, source=C4.LANCZOS)
    free = []
    for _ in range(6):
        c = G.context("SYN")
        c.estimate_lmax(1, STEPS)
        c.estimate_lmax(0, 64)
        set4(c, cfg)
        G.smooth(c, 1, u0, rhs, True)
        c.set_level_matrix(1, ha.level_matrices[1])
        G.smooth(c, 1, u0, rhs, False)
        c.reset(2)
        G.load(c, h)
        G.smooth(c, 1, u0, rhs, True)
        c.close()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    print("\n[cheb4-gpu] free device memory after each round, relative to the first:", [f - free[0] for f in free])
    assert free[-1] == free[0], free


# ------------------------------------------------------------------------------------------------ the driver

def test_driver_prm_keys():
    """8 atoms, two adaptive cycles, the smoother selected through the prm keys: every solve reaches the outer tolerance
    1e-8 ||rhs||.  The iteration counts are printed for DESIGN.md section 30; which is smaller is not asserted"""
    S = pkg().step50
    base = dict(left=0, right=1, mesh_size=0.25, vacuum=4, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=2, r_c=0.5, cutoff=3.5,
                rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="Chebyshev", cheb_degree=3)
    runs = {"first kind, Gershgorin": {}, "first kind, Lanczos": dict(cheb_estimate="Lanczos"),
            "fourth kind, Gershgorin": dict(cheb_polynomial="fourth kind"),
            "fourth kind, Lanczos": dict(cheb_polynomial="fourth kind", cheb_estimate="Lanczos", cheb_lanczos_steps=12, cheb_safety=1.15)}
    counts = {}
    for what, extra in runs.items():
        p = S.Problem(S.prm_text(**base, **extra))
        p.set_nacl_atoms(1)
        counts[what] = []
        for cycle in (0, 1):
            r = p.run_cycle(cycle)
            assert r["convergence_value"] <= 1e-8 * r["rhs_l2"], (what, cycle, r["convergence_value"], r["rhs_l2"])
            counts[what].append(r["cg_iterations"])
        if "Lanczos" in what:
            info = capi().Context.view(p.gmg_context()).get_chebyshev(1)
            assert info["lmax_source"] == 1 and info["steps_run"] > 0 and 1.0 <= info["lmax"] <= info["gershgorin"]
            assert info["polynomial"] == (1 if "fourth" in what else 0)
        p.close()
    print("\n[cheb4-gpu] driver, 8 atoms, outer CG iterations of cycles 0 and 1: " + ", ".join(f"{k}: {v}" for k, v in counts.items()))
