"""tests/cheb4_reference.py proven on the CPU: the three evaluations of the fourth-kind smoother agree,
every mutation of the derivation is seen at SENSITIVITY tolerances, the Lanczos bound brackets the true lambda_max, the
breakdown case, and that the library declares what the GPU tests call.  The figures are printed: run with -s to read them."""
import os
import re

import numpy as np
import pytest

import cheb4_reference as C4
import mg_cases as K
import mg_reference as R
from gpu_util import capi, pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEGREES = (1, 2, 3, 4, 5)


# ------------------------------------------------------------------------------------------------ the polynomial itself

def test_recurrence_equals_closed_form():
    """the scalar recurrence against 1 - x q(x) = W_k(1 - 2 x / lambda) / (2 k + 1), W_k(cos t) = sin((k + 1/2) t) / sin(t / 2), on
    (0, lambda): the residual polynomials agree to 2e-15 of p(0) = 1 (section 30), and W_k vanishes at the roots x_j"""
    lam = 1.7
    x = np.linspace(0.01, lam - 0.01, 301)
    for k in DEGREES:
        d = 4 / (3 * lam) * np.ones_like(x)      # S r for B = 1, A = x, r = 1
        y = d.copy()
        for j in range(1, k):
            d = (2 * j - 1) / (2 * j + 3) * d + (8 * j + 4) / ((2 * j + 3) * lam) * (1 - x * y)
            y = y + d
        t = np.arccos(1 - 2 * x / lam)
        p = np.sin((k + 0.5) * t) / np.sin(t / 2) / (2 * k + 1)   # the residual polynomial 1 - x q(x); p(0) = 1 is its scale
        assert np.abs((1 - x * y) - p).max() <= 2e-15, k
        roots = lam * (1 - np.cos(np.arange(1, k + 1) * np.pi / (k + 0.5))) / 2
        tr = np.arccos(1 - 2 * roots / lam)
        assert np.abs(np.sin((k + 0.5) * tr) / np.sin(tr / 2)).max() <= 64 * R.U * (2 * k + 1)


EIG_FACTOR = 64.0   # the eigen-decomposition against the roots, in u ||ref||: see test_three_evaluations


@pytest.mark.parametrize("name,level", K.SMOOTH_LEVELS)
def test_three_evaluations(name, level):
    """the recurrence (f64), the product over the roots (ld) and the eigen-decomposition agree for degrees 1 to 5 under the
    Gershgorin bound, the Lanczos bound and a user bound.
    Recurrence against roots: the tolerance of section 16, TOL_FACTOR x S x ||ref||, S the spread of these two (no smaller
    than u); what the assertion can fail on is S itself, which has to stay a rounding scale: at most 8 u.
    Eigen-decomposition against roots: S holds nothing of eigh's rounding (its eigenpairs carry a backward error of p(n) u
    ||A|| with a modest p(n), and q(x) = (1 - p(x)) / x divides by the small eigenvalues), so that pair cannot be held to
    TOL_FACTOR S; it is held to EIG_FACTOR u ||ref|| = TOL_FACTOR u ||ref||, the tolerance of a case whose tiers agree to the
    last bit -- the allowance the project gives one differently ordered fp64 evaluation.  This is a deviation from "within
    the tolerance" for this pair alone, recorded in DESIGN.md section 30; the figures are printed"""
    H = C4.hierarchy4(name)
    r = K.smoother_vectors(name, level)[1][:, None]
    worst = [0.0, 0.0, 0.0]
    for k in DEGREES:
        for cfg in (C4.Config4(degree=k), C4.Config4(degree=k, source=C4.LANCZOS), C4.Config4(degree=k, lmax=1.7)):
            f, l = (H.levels(t)[level].cheb4(cfg, r.astype(H.levels(t)[level].dtype)) for t in R.TIERS)
            e = C4.cheb4_by_eig(H.A[level], H.levels("ld")[level].lam(cfg), k, r)
            S = R.spread(f, l)
            tol = float(R.tolerance(S, l))
            scale = float(np.linalg.norm(R.as_f64(l)))
            df, de = float(np.linalg.norm(f - R.as_f64(l))), float(np.linalg.norm(e - R.as_f64(l)))
            worst = [max(worst[0], df / scale), max(worst[1], de / scale), max(worst[2], S)]
            assert df <= tol and S <= 8 * R.U, (cfg.label(), df, tol, S)
            assert de <= EIG_FACTOR * R.U * scale, (cfg.label(), de / scale / R.U)
    print(f"\n[cheb4] three evaluations {name} level {level}: recurrence - roots {worst[0] / R.U:.1f} u (spread {worst[2] / R.U:.1f} u), "
          f"eigen - roots {worst[1] / R.U:.1f} u")


# ------------------------------------------------------------------------------------------------ sensitivity

def sensitivity_cases():
    """(name, level, cfg, from_zero, mutation): every pair on which the mutation changes the derivation at all.  j_shift needs a
    step j >= 1 (degree >= 2); no_safety needs the Lanczos source.  Two steps, apply and smooth."""
    out = []
    for name, level in K.SMOOTH_LEVELS:
        for k in DEGREES:
            for source in (C4.GERSHGORIN, C4.LANCZOS):
                cfg = C4.Config4(degree=k, steps=2, source=source)
                muts = ["first_kind_alpha0", "no_four_thirds"] + (["j_shift"] if k >= 2 else []) + (["no_safety"] if source == C4.LANCZOS else [])
                out += [(name, level, cfg, fz, m) for fz in (True, False) for m in muts]
    return out


def test_mutations_are_seen():
    """every mutation misses by SENSITIVITY tolerances on the kept pairs; the dropped pairs are recorded and at most one in
    four.  On these cases none is dropped (396 pairs, the smallest ratio 1e11).  The only pair that could be is no_safety on a
    level whose Ritz value exceeds its Gershgorin bound: there the minimum leaves the bound where it was"""
    low, dropped, cases = {}, [], sensitivity_cases()
    for name, level, cfg, fz, mut in cases:
        H = C4.hierarchy4(name)
        u0, rhs = K.smoother_vectors(name, level)
        ref = C4.smoother_reference(name, level, cfg, fz)
        true = H.smooth("f64", cfg, level, u0, rhs, fz)
        ratio = float(np.linalg.norm(H.smooth("f64", cfg.with_mut4(mut), level, u0, rhs, fz) - true)) / ref.tol
        if ratio >= R.SENSITIVITY:
            low[mut] = min(low.get(mut, np.inf), ratio)
        else:
            dropped.append((name, level, cfg.label(), fz, mut, ratio))
    print(f"\n[cheb4] sensitivity: {len(cases)} pairs, {len(dropped)} dropped; smallest kept difference / tolerance: "
          + ", ".join(f"{m} {v:.1e}" for m, v in sorted(low.items())))
    for d in dropped:
        print(f"[cheb4]   dropped {d}")
    assert set(low) == set(C4.MUTATIONS4)
    assert 4 * len(dropped) <= len(cases), (len(dropped), len(cases))
    assert all(d[4] == "no_safety" for d in dropped), dropped


# ------------------------------------------------------------------------------------------------ the bound

LANCZOS_STEPS = 10   # the library's default; no case needed more (a case that did would be listed here with its count)
# D^-1 A of A3 level 2 (250 rows, a patch of two cells' depth) has 7 distinct eigenvalues: the recurrence is exact after 7 steps,
# rho_7 / rho_0 is 6e-39 in fp64 (threshold 2^-100 = 8e-31) and the Ritz value is lambda_max itself
EXACT_AFTER = {("A3", 2): 7}


def true_lmax(name, level):
    A = K.hierarchy(name)[1].A[level]
    d = A.diagonal()
    if A.shape[0] <= 4096:
        a = A.toarray() / np.sqrt(d)[:, None] / np.sqrt(d)[None, :]
        return float(np.linalg.eigvalsh((a + a.T) / 2)[-1])
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    s = sp.diags(1 / np.sqrt(d))
    return float(spla.eigsh((s @ A @ s).tocsr(), k=1, which="LA", tol=1e-12, return_eigenvectors=False)[0])


@pytest.mark.parametrize("name,level", K.SMOOTH_LEVELS + [(K.LAT, 1)])
def test_bound_brackets_lambda_max(name, level):
    """ritz <= lambda_max (the Ritz values of a symmetric operator lie inside its spectrum) up to the rounding scale of the
    case, and safety x ritz >= lambda_max with the default 10 steps and the default factor 1.2"""
    ref = C4.lanczos_reference(name, level, LANCZOS_STEPS)
    lmax = true_lmax(name, level)
    print(f"\n[cheb4] bound {name} level {level}: lambda_max {lmax:.6f}, ritz({ref.steps_run}) {ref.ritz:.6f} = {ref.ritz / lmax:.4f} lambda_max, "
          f"Gershgorin {ref.gershgorin:.6f}, spread of alpha {ref.S_alpha:.1e} beta {ref.S_beta:.1e} ritz {ref.S_ritz:.1e}")
    assert ref.steps_run == EXACT_AFTER.get((name, level), LANCZOS_STEPS)
    assert ref.ritz <= lmax * (1 + 4096 * R.U) + ref.tol_ritz
    assert 1.2 * ref.ritz >= lmax
    assert ref.gershgorin >= lmax * (1 - 64 * R.U)


def test_start_vector():
    r = C4.start_vector(5)
    want = [((((i + 1) * 2654435761) % 2 ** 32) >> 8) / 2 ** 24 - 0.5 for i in range(5)]
    assert r.tolist() == want and np.abs(C4.start_vector(100000)).max() <= 0.5


def test_breakdown_on_identity():
    """hier3 level 1: 27 rows, every one a boundary row, D^-1 A = I: one step, ritz 1, in both tiers.  (r / a_ii) a_ii is r up to
    a rounding, so alpha is 1 and rho_1 is 0 up to roundings: beta is below the breakdown threshold 2^-100, not exactly 0)"""
    H = C4.hierarchy4("hier3")
    assert H.rows[1] == 27
    for t in R.TIERS:
        a, b = H.levels(t)[1].lanczos(10)
        assert len(a) == 1 and abs(float(a[0]) - 1.0) <= 8 * R.U and 0.0 <= float(b[0]) <= 2.0 ** -100
        assert abs(C4.ritz(a, b) - 1.0) <= 8 * R.U


# ------------------------------------------------------------------------------------------------ the library's surface

NEW_SYMBOLS = ("gmg_set_chebyshev", "gmg_estimate_lmax", "gmg_get_chebyshev")
OPTION_KEYS = ("cheb_polynomial", "cheb_lmax_source", "cheb_lanczos_steps", "cheb_safety", "cheb_degree")


def test_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "gmg_coulomb.h")).read()
    for name, value in (("GMG_CHEB_FIRST_KIND", 0), ("GMG_CHEB_FOURTH_KIND", 1), ("GMG_CHEB_LMAX_GERSHGORIN", 0), ("GMG_CHEB_LMAX_LANCZOS", 1)):
        assert re.search(rf"#define {name} {value}\b", text), name
    pkg().build.build_device()
    lib = capi().load()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bint {s}\(", text) and hasattr(lib, s) and s in capi().SYMBOLS, s
    assert (capi().CHEB_FIRST_KIND, capi().CHEB_FOURTH_KIND, capi().CHEB_LMAX_GERSHGORIN, capi().CHEB_LMAX_LANCZOS) == (0, 1, 0, 1)


def test_option_keys_default_to_unset():
    """the keys exist in gmg_set_option and the context's defaults are the behaviour before them: first kind, Gershgorin, 10
    steps, 1.2, no degree override (what a context reports on the device: tests/test_gpu_chebyshev4.py test_defaults)"""
    src = open(os.path.join(ROOT, pkg().__name__, "csrc", "gmg_coulomb.hip")).read()
    for key in OPTION_KEYS:
        assert f'k == "{key}"' in src, key
    assert re.search(r"cheb_polynomial = GMG_CHEB_FIRST_KIND, cheb_lmax_source = GMG_CHEB_LMAX_GERSHGORIN, cheb_lanczos_steps = 10;", src)
    assert re.search(r"double cheb_safety = 1\.2;", src) and re.search(r"int cheb_degree_opt = 0;", src)


def test_driver_defaults_print_the_same_log(golden_dir):
    """a host driver run with the four prm keys written out at their defaults prints the log of a run without them"""
    pkg().build.build_all()
    S = pkg().step50
    base = dict(left=0, right=1, mesh_size=0.25, vacuum=1, problem="GaussianCharges", dim=3, bc="Exact", cycles=2, r_c=0.5, cutoff=3.5,
                rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="Chebyshev")
    logs = []
    for extra in ({}, dict(cheb_polynomial="first kind", cheb_estimate="Gershgorin", cheb_lanczos_steps=10, cheb_safety=1.2)):
        p = S.Problem(S.prm_text(**base, **extra))
        p.read_lammps(os.path.join(golden_dir, "atom_n1_2.data"))
        p.run_cycle(0, on_device=False)
        logs.append(p.log())
        p.close()
    assert logs[0] == logs[1] and len(logs[0]) > 0
    for bad in (dict(cheb_polynomial="second kind"), dict(cheb_estimate="power"), dict(cheb_lanczos_steps=0), dict(cheb_safety=0.5)):
        with pytest.raises(RuntimeError):
            S.Problem(S.prm_text(**base, **bad))
