"""One capi.Context used the way the host driver and bench.py use it: reset and loaded again, loaded again without a reset, one
operator or one list replaced in place.  Everything a context derives from an operator or a copy list --
the inverse tables of the fused copies, 1 / diag, the Gershgorin bound, the SSOR plan and its pre-pass operands, the transposes,
the work vectors, the coarse CG's vectors, the SELL / hybrid copies, the direct coarse solver's tables, the system's 1 / diag --
must follow what it was derived from.  Every step of every sequence is checked two ways:

  (a) against tests/mg_reference.py of the hierarchy the context holds at that moment, by test_gpu_mg_reference.check_vcycle with
      its tolerances (64 S_case ||ref|| + the coarse allowance);
  (b) against a fresh context given only the final configuration, bit for bit (the library's results are deterministic).

The twins and substitutions of tests/mg_cases.py have SYN's sizes: a stale table faults nowhere, it computes SYN's M, which
tests/test_mg_reference_cpu.py proves to be 1000 tolerances or more from the reference of every case here
(test_reuse_case_discriminates, test_reuse_twin_stale_tables).  Each sequence runs with the fused copies and with option
disable_vcycle_fused.  Each test prints its worst error / tolerance ("[reuse]", run with -s)."""
from types import SimpleNamespace

import numpy as np
import pytest

import cg_reference as CG
import mg_cases as K
import mg_reference as R
import test_gpu_coarse_cg as OC
import test_gpu_hybrid_spmv as HY
import test_gpu_mg_reference as G
from gpu_util import capi
from oracle import gmg_oracle as go

pytestmark = pytest.mark.gpu

TAU = G.TAU
CFGS = [R.Config(kind=R.SSOR, steps=2), R.Config(kind=R.JACOBI, steps=3, degree=3), R.Config(kind=R.CHEBYSHEV, steps=2, degree=2),
        R.Config(kind=R.SSOR, steps=0)]
assert all(cfg in K.VCYCLE_CONFIGS for cfg in CFGS) and all(cfg in CFGS for cfg in K.LAYOUT_CFGS)
UNFUSED = pytest.mark.parametrize("unfused", [0, 1], ids=["fused", "disable_vcycle_fused"])


def cfgs_of(name):
    return K.LAYOUT_CFGS if name == K.LAT else CFGS


def options(unfused):
    return (("disable_vcycle_fused", 1),) if unfused else ()


def smoother_runs(c, name):
    """gmg_smoother_step on level 1, apply and smooth, for the configurations with a step to run"""
    u0, rhs = K.smoother_vectors(name, 1)
    out = {}
    for cfg in [cfg for cfg in CFGS if cfg.steps > 0]:
        G.set_smoother(c, cfg)
        for from_zero in (True, False):
            out[cfg, from_zero] = G.smooth(c, 1, u0, rhs, from_zero)
    return out


def coarse_vector(name):
    n0 = K.hierarchy(name)[1].rows[0]
    return np.random.default_rng(17 + n0).standard_normal(n0)


def coarse_run(c, name):
    d = coarse_vector(name)
    c.set_coarse(TAU, 1000)
    vd, vu = c.vector(len(d), d), c.vector(len(d))
    it, res, rc = c.coarse_solve(vu, vd)
    u = vu.download()
    vd.free()
    vu.free()
    return SimpleNamespace(u=u, iterations=it, res=res, rc=rc)


@pytest.fixture(scope="module")
def fresh():
    """(b): what a context that never held anything else gives.  get(name, way, unfused) -> namespace(v {cfg: [n_sys, k]},
    s {(cfg, from_zero): [n_1]} and coarse for the SYN family); way: "csr", "lattice-cg" or "lattice-direct" (level 0 formed
    by gmg_set_level_matrix_lattice).  Computed once per key and shared."""
    made = {}

    def get(name, way="csr", unfused=0):
        key = (name, way, unfused)
        if key not in made:
            lattice = None if way == "csr" else K.level0_lattice(name)[:2]
            c = G.context(name, options=options(unfused), lattice=lattice)
            if way == "lattice-direct":
                c.set_coarse_solver(capi().COARSE_DIRECT)
            c.set_coarse(TAU, 1000)
            out = SimpleNamespace(v={}, s={}, coarse=None)
            for cfg in cfgs_of(name):
                G.set_smoother(c, cfg)
                out.v[cfg] = G.run_sources(c, name)
            if name.startswith("SYN"):
                out.s = smoother_runs(c, name)
                out.coarse = coarse_run(c, name)
            c.close()
            made[key] = out
        return made[key]

    return get


def check_step(c, name, fresh, unfused, what, worst, way="csr"):
    """gmg_precondition over all of K.vcycle_sources(name) for every configuration: (a) and (b)"""
    H = K.hierarchy(name)[1]
    c.set_coarse(TAU, 1000)
    for cfg in cfgs_of(name):
        G.set_smoother(c, cfg)
        got = G.run_sources(c, name)
        if way == "lattice-direct":
            allowance = H.direct_allowance(cfg, K.level0_lattice(name)[0], K.vcycle_reference(name, cfg).coarse_norm)
        else:
            allowance = H.cg_allowance(cfg, TAU)
        worst[0] = max(worst[0], G.check_vcycle(name, cfg, got, allowance, what)[0])
        want = fresh(name, way, unfused).v[cfg]
        assert np.array_equal(got, want), (what, cfg.label(), "not the bits of a fresh context", float(np.abs(got - want).max()))


def check_smoother(c, name, fresh, unfused, what, worst):
    got = smoother_runs(c, name)
    for (cfg, from_zero), val in got.items():
        ref = K.smoother_reference(name, 1, cfg, from_zero)
        err = float(np.linalg.norm(val - ref.ref))
        worst[0] = max(worst[0], err / ref.tol)
        assert err <= ref.tol, (what, cfg.label(), from_zero, err, ref.tol)
        assert np.array_equal(val, fresh(name, "csr", unfused).s[cfg, from_zero]), (what, cfg.label(), from_zero)


def check_coarse(c, name, fresh, unfused, what, worst):
    """gmg_coarse_solve at tau = 1e-10 against A_0^-1 d of the reference's longdouble tier.  The CG stops on its recurrence's
    residual, which mg_reference.cg_floor puts within 64 u kappa_2 ||d|| of the true one; the true residual r leaves
    ||u - A_0^-1 d|| <= ||r|| / lambda_min(A_0) (the two terms of the coarse allowances of mg_reference, before ||T||)."""
    H = K.hierarchy(name)[1]
    d = coarse_vector(name)
    got = coarse_run(c, name)
    exact = R.as_f64(H.coarse_exact("ld", d.astype(np.longdouble)[:, None])[:, 0])
    resid = TAU + H.cg_floor() * float(np.linalg.norm(d))
    err, tol = float(np.linalg.norm(got.u - exact)), resid / H.coarse_spectrum[0]
    worst[0] = max(worst[0], err / tol)
    assert got.rc == 0 and got.res <= TAU and err <= tol, (what, got.rc, got.res, err, tol)
    assert float(np.linalg.norm(H.A[0] @ got.u - d)) <= resid, what
    want = fresh(name, "csr", unfused).coarse
    assert got.iterations == want.iterations and np.array_equal(got.u, want.u), (what, got.iterations, want.iterations)


def report(what, unfused, worst):
    print(f"\n[reuse] {what}{' (disable_vcycle_fused)' if unfused else ''}: error / tolerance max {worst[0]:.3f}")


# ------------------------------------------------------------------------------------------------ 1-3: the copy lists

@UNFUSED
def test_reset_then_twin(fresh, unfused):
    """Sequence 1: SYN, reset, SYN-T, reset, SYN.  Every level's copy_version restarts at 0 with gmg_reset, so SYN-T repeats
    the signature (n_sys, then n_vec, n_copy, copy_version per level) of the tables built for SYN: a context that kept the
    tables across the reset gathers and scatters through SYN's lists (DESIGN.md section 29 has the ratio it then shows)."""
    worst = [0.0]
    c = G.context("SYN", options=options(unfused))
    check_step(c, "SYN", fresh, unfused, "SYN", [0.0])   # (the start: not part of the figure reported)
    for name in (K.REUSE_TWIN, "SYN"):
        c.reset(2)
        c.load_hierarchy(K.hierarchy(name)[0])
        check_step(c, name, fresh, unfused, f"reset, {name}", worst)
    c.close()
    report("reset then twin", unfused, worst)


@UNFUSED
def test_reload_without_reset(fresh, unfused):
    """Sequence 2: SYN and then SYN-T through load_hierarchy twice.  copy_version advances: the path that always worked."""
    worst = [0.0]
    c = G.context("SYN", options=options(unfused))
    check_step(c, "SYN", fresh, unfused, "SYN", [0.0])   # (the start: not part of the figure reported)
    c.load_hierarchy(K.hierarchy(K.REUSE_TWIN)[0])
    check_step(c, K.REUSE_TWIN, fresh, unfused, "SYN-T loaded over SYN", worst)
    c.close()
    report("reload without reset", unfused, worst)


@UNFUSED
def test_lists_alone(fresh, unfused):
    """Sequence 3: only gmg_set_copy_indices, both levels, with SYN-T's lists on a context that holds SYN (the operators are
    equal: it now holds SYN-T), coarse level first; then SYN's lists again, fine level first -- the tables are built with the
    finest level's list, so the level-0 list that follows is seen by the signature at the next V-cycle alone."""
    worst = [0.0]
    c = G.context("SYN", options=options(unfused))
    check_step(c, "SYN", fresh, unfused, "SYN", [0.0])   # (the start: not part of the figure reported)
    for name, order in ((K.REUSE_TWIN, (0, 1)), ("SYN", (1, 0))):
        h = K.hierarchy(name)[0]
        for l in order:
            c.set_copy_indices(l, h.copy_global[l], h.copy_level[l])
        check_step(c, name, fresh, unfused, f"lists of {name}, levels {order}", worst)
    c.close()
    report("lists alone", unfused, worst)


# ------------------------------------------------------------------------------------------------ 4: one operator in place

def replace(c, name, h):
    if name == "SYN-A1":
        c.set_level_matrix(1, h.level_matrices[1])
    elif name == "SYN-A0":
        c.set_level_matrix(0, h.level_matrices[0])
    elif name == "SYN-I":
        c.set_edge_matrix(1, h.edge_matrices[1])
    else:
        c.set_prolongation(0, h.prolongations[0])


@UNFUSED
@pytest.mark.parametrize("name", K.REUSE_SUBSTITUTIONS)
def test_one_operator_replaced(fresh, name, unfused):
    """Sequence 4: from SYN one call of gmg_set_level_matrix(1) / (0), gmg_set_edge_matrix(1) or gmg_set_prolongation(0) gives
    SYN-A1 / SYN-A0 / SYN-I / SYN-P; the V-cycles, the smoother steps on level 1 and (level 0 replaced) gmg_coarse_solve.  The
    same call with SYN's operator then gives SYN again."""
    worst = [0.0]
    c = G.context("SYN", options=options(unfused))
    check_step(c, "SYN", fresh, unfused, "SYN", [0.0])   # (the start: not part of the figure reported)
    for now in (name, "SYN"):
        replace(c, name, K.hierarchy(now)[0])
        check_step(c, now, fresh, unfused, f"{name}: holds {now}", worst)
        check_smoother(c, now, fresh, unfused, f"{name}: holds {now}", worst)
        if name == "SYN-A0":
            check_coarse(c, now, fresh, unfused, f"{name}: holds {now}", worst)
    c.close()
    report(f"one operator replaced, {name}", unfused, worst)


# ------------------------------------------------------------------------------------------------ 5: other sizes, level counts

@UNFUSED
def test_sizes_and_level_counts_with_reset(fresh, unfused):
    """Sequence 5, first half: A3 (3 levels), reset(2), A2, reset(3), B3, reset(2), SYN"""
    worst = [0.0]
    c = G.context("A3", options=options(unfused))
    check_step(c, "A3", fresh, unfused, "A3", worst)
    for name in ("A2", "B3", "SYN"):
        h = K.hierarchy(name)[0]
        c.reset(len(h.level_matrices))
        c.load_hierarchy(h)
        check_step(c, name, fresh, unfused, f"reset, {name}", worst)
    c.close()
    report("A3, A2, B3, SYN with resets", unfused, worst)


@UNFUSED
def test_sizes_without_reset(fresh, unfused):
    """Sequence 5, second half: SYN, LAT, SYN-T on a 2-level context without a reset.  LAT's level operators take the SELL /
    pattern / lattice layouts, so one DevCSR changes layout both ways; LAT runs K.LAYOUT_CFGS only."""
    worst = [0.0]
    c = G.context("SYN", options=options(unfused))
    check_step(c, "SYN", fresh, unfused, "SYN", [0.0])   # (the start: not part of the figure reported)
    for name in (K.LAT, K.REUSE_TWIN):
        c.load_hierarchy(K.hierarchy(name)[0])
        check_step(c, name, fresh, unfused, f"{name} loaded over the last", worst)
    c.close()
    report("SYN, LAT, SYN-T without reset", unfused, worst)


# ------------------------------------------------------------------------------------------------ 6: the direct coarse solver

@UNFUSED
def test_direct_coarse_solver_across_replacement(fresh, unfused):
    """Sequence 6: A2 with level 0 formed by gmg_set_level_matrix_lattice; COARSE_DIRECT selected (H.direct_allowance); level 0
    formed again: the coarse CG is selected again, as include/gmg_coulomb.h says of gmg_set_coarse_solver (H.cg_allowance)."""
    C = capi()
    worst = [0.0]
    shape, Ke, _ = K.level0_lattice("A2")
    c = G.context("A2", options=options(unfused), lattice=(shape, Ke))
    check_step(c, "A2", fresh, unfused, "lattice, CG", worst, way="lattice-cg")
    assert int(c.stats().coarse_solver) == C.COARSE_CG           # (gmg_stats.coarse_solver: of the last coarse solve)
    c.set_coarse_solver(C.COARSE_DIRECT)
    check_step(c, "A2", fresh, unfused, "lattice, direct", worst, way="lattice-direct")
    assert int(c.stats().coarse_solver) == C.COARSE_DIRECT
    c.set_level_matrix_lattice(0, shape, Ke)
    check_step(c, "A2", fresh, unfused, "lattice formed again, CG", worst, way="lattice-cg")
    assert int(c.stats().coarse_solver) == C.COARSE_CG
    c.close()
    report("direct coarse solver across replacement", unfused, worst)


# ------------------------------------------------------------------------------------------------ 7: the system matrix

def hybrid_operator():
    """test_gpu_hybrid_spmv.banded with one wide row (its "wide row in the middle of slice 3": layout hybrid), the diagonal
    set to 256: the off-diagonals of a row sum to less than 84 x 8 / 3 = 224 in magnitude, so every row is strictly
    diagonally dominant with a positive diagonal and the Jacobi-preconditioned operator is within 0.875 of the identity in the
    infinity norm -- the outer CG and its reference then take the same few, well-separated steps"""
    m = HY.banded(n=1088, wide_rows=(3 * 64 + 32,))
    row = np.repeat(np.arange(m.n_rows), np.diff(m.rowptr))
    m.val = np.where(m.col == row, 256.0, m.val)
    assert np.array_equal(np.bincount(row[m.col == row], minlength=m.n_rows), np.ones(m.n_rows, dtype=np.int64))
    return m


def stop_case(m, b):
    """(tol, reference) of the Jacobi-preconditioned solve that stops at an iteration cg_reference.target_tol accepts: the
    residuals before it are 1.05 tol or more and its own tol / 1.05 or less, so no rounding moves the stopping iteration"""
    hist = CG.cg(m, b, 0.0, 40, precond=CG.jacobi, keep_steps=False).history
    for k in range(8, 30):
        try:
            tol = CG.target_tol(hist, k)
        except ValueError:
            continue
        return tol, CG.cg(m, b, tol, 500, precond=CG.jacobi)
    raise AssertionError("no targetable iteration")


def system_cases():
    m0, _ = CG.operator("csr")
    m1 = SimpleNamespace(**vars(m0))
    m1.val = m0.val * 0.375
    m2 = hybrid_operator()
    b0, b2 = CG.rhs("csr"), np.random.default_rng(1088).standard_normal(1088)
    return [("csr", m0, b0, False), ("csr, values x 0.375", m1, b0, False), ("banded", m2, b2, True), ("csr again", m0, b0, False)]


def system_checks(c, m, b, tol, ref, what):
    """spmv, precondition_jacobi and cg_solve of the system matrix the context holds -> (jacobi result, cg result)"""
    C = capi()
    n = m.n_rows
    x = np.random.default_rng(n + 1).standard_normal(n)
    vx, vy = c.vector(n, x), c.vector(n, np.full(n, np.nan))
    c.spmv(C.SYSTEM, vy, vx)
    assert np.array_equal(vy.download(), go.spmv(m, x)), (what, "spmv")
    vy.upload(np.full(n, np.nan))
    c.precondition_jacobi(0.6, vy, vx)
    jac = vy.download()
    vx.free()
    vy.free()
    assert np.array_equal(jac, (0.6 * x) * (1.0 / CG.diagonal(m))), (what, "precondition_jacobi")   # (a x) z: one rounding each
    norm_b = float(CG.cg(m, b, np.inf, 0, tier="ld").res)
    r = OC.outer_solve(c, b, np.zeros(n), tol, norm_b, 500, "jacobi")
    OC.outer_check(r, ref, ("system replaced", what))
    r["ratio"] = float(np.abs(r["x"] - ref.x).max() / (CG.x_tolerance("csr") * np.abs(ref.x).max()))   # (the figure outer_check asserts on)
    return jac, r


def test_system_matrix_replaced(capfd):
    """Sequence 7: on a one-level context gmg_set_system_matrix with cg_reference's "csr" operator, the same pattern with the
    values scaled, a banded operator that takes layout hybrid, and the first again.  After each: gmg_spmv(SYSTEM) is
    oracle.spmv's bits, gmg_precondition_jacobi(0.6) is (0.6 x) (1 / a_ii) to the bit, and gmg_cg_solve with PRECOND_JACOBI
    follows cg_reference.cg by test_gpu_coarse_cg.outer_check; the last two are also a fresh context's bits."""
    cases = [(what, m, b, hyb) + stop_case(m, b) for what, m, b, hyb in system_cases()]
    for what, m, b, hyb, tol, ref in cases:   # the rule of outer_check was measured on "csr": it holds for a case whose own tiers agree as well
        assert ref.status == CG.OK and 8 <= ref.iterations < 30, (what, ref.iterations)
        ld = CG.cg(m, b, tol, 500, precond=CG.jacobi, tier="ld")
        assert ld.iterations == ref.iterations and np.abs(ld.x - ref.x).max() <= CG.spread() * np.abs(ref.x).max(), what
    worst = 0.0
    c = capi().Context(1)
    c.set_option("debug_upload", 1)
    for what, m, b, hyb, tol, ref in cases:
        capfd.readouterr()
        c.set_system_matrix(m)
        err = capfd.readouterr().err
        assert ("[gmg]   layout hybrid" in err) == hyb, (what, err)
        jac, r = system_checks(c, m, b, tol, ref, what)
        f = capi().Context(1)
        f.set_system_matrix(m)
        fjac, fr = system_checks(f, m, b, tol, ref, what + ", fresh")
        f.close()
        assert np.array_equal(jac, fjac) and np.array_equal(r["x"], fr["x"]) and r["iterations"] == fr["iterations"], what
        worst = max(worst, r["ratio"])
    c.close()
    with capfd.disabled():
        print(f"\n[reuse] system matrix replaced: |x - ref| / tolerance max {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 8: a refused replacement

@UNFUSED
def test_refused_replacement(fresh, unfused):
    """Sequence 8: gmg_set_level_matrix(1) with a column out of range is refused with ERR_INVALID on the host, before any
    launch.  include/gmg_coulomb.h: the level is then WITHOUT an operator (not with the previous one), gmg_precondition returns
    ERR_INVALID until a valid matrix is set, and the context is then as if the refused call had not been made."""
    C = capi()
    worst = [0.0]
    h = K.hierarchy("SYN")[0]
    c = G.context("SYN", options=options(unfused))
    check_step(c, "SYN", fresh, unfused, "SYN", [0.0])   # (the start: not part of the figure reported)
    bad = SimpleNamespace(**vars(h.level_matrices[1]))
    bad.col = bad.col.copy()
    bad.col[len(bad.col) // 2] = bad.n_cols
    with pytest.raises(C.GMGError) as e:
        c.set_level_matrix(1, bad)
    assert e.value.code == C.ERR_INVALID
    src, labels, dst0 = K.vcycle_sources("SYN")
    vs, vd = c.vector(len(dst0), src[:, 0]), c.vector(len(dst0), dst0)
    with pytest.raises(C.GMGError) as e:
        c.precondition(vd, vs)
    assert e.value.code == C.ERR_INVALID
    vs.free()
    vd.free()
    c.set_level_matrix(1, h.level_matrices[1])
    check_step(c, "SYN", fresh, unfused, "the good matrix after the refused one", worst)
    check_smoother(c, "SYN", fresh, unfused, "the good matrix after the refused one", worst)
    c.close()
    report("refused replacement", unfused, worst)
