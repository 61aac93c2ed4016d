"""tests/mg_reference.py proven on the CPU: the oracle against it on every case tests/test_gpu_mg_reference.py
runs, with the same tolerance rule; what the dense M must satisfy; every mutation of the definition seen at 1000 tolerances or
more on every case it applies to.  The figures (S_case, the oracle's error / tolerance, the sensitivity ratios) are printed:
run with -s to read them."""
import numpy as np
import pytest

import mg_cases as K
import mg_reference as R
from oracle import gmg_oracle as go
from oracle import step50_oracle as so

TAU = 1e-10   # the coarse CG's tolerance of the oracle and of the device's default


def oracle_mg(h, cfg):
    return go.OracleMG(h, smoother=cfg.kind, omega=cfg.omega, steps=cfg.steps, cheb_degree=cfg.degree, cheb_ratio=cfg.ratio,
                       cheb_lmax=cfg.lmax, ssor_blocks=cfg.blocks, coarse_tol=TAU)


def test_fixture_sizes():
    for name, (_, _, _, _, rows, edges, copies, n_sys, n_con) in K.ADAPTIVE.items():
        h, H = K.hierarchy(name)   # asserts the table of DESIGN.md section 16
        assert H.rows == rows and H.n_sys == n_sys
        assert len(K.zero_rows(name)) > 0 and len(K.edge_dofs(name)) == len(rows) - 1
    h, H = K.hierarchy("SYN")
    assert H.rows[1] % 64 == 17 and not np.array_equal(np.sort(H.copy_global[1]), H.copy_global[1])
    assert K.hierarchy("hier3")[1].n_levels == 5 and all(e is None or e.nnz == 0 for e in K.hierarchy("hier3")[0].edge_matrices)


@pytest.mark.parametrize("name,level", K.SMOOTH_LEVELS)
def test_oracle_smoother_against_reference(name, level):
    h, H = K.hierarchy(name)
    u0, rhs = K.smoother_vectors(name, level)
    worst, S = 0.0, 0.0
    for cfg in K.smoother_configs(name, level):
        for from_zero in (True, False):
            ref = K.smoother_reference(name, level, cfg, from_zero)
            S = max(S, ref.S)
            if cfg.bounds:
                continue   # the oracle has no caller-given partition; tests/test_gpu_ssor_partition.py composes one
            err = float(np.linalg.norm(oracle_mg(h, cfg).smooth(level, u0, rhs, from_zero) - ref.ref))
            worst = max(worst, err / ref.tol)
            assert err <= ref.tol, (cfg.label(), from_zero, err, ref.tol)
    print(f"\n[mg] smoother {name} level {level}: S_case max {S:.2e}, oracle error / tolerance max {worst:.3f}")


@pytest.mark.parametrize("name", K.NAMES)
def test_oracle_vcycle_against_reference(name):
    h, H = K.hierarchy(name)
    src, labels, dst0 = K.vcycle_sources(name)
    worst, S = 0.0, 0.0
    for cfg in K.VCYCLE_CONFIGS:
        ref = K.vcycle_reference(name, cfg)
        tol = ref.tol + H.cg_allowance(cfg, TAU)
        o = oracle_mg(h, cfg)
        for j, lab in enumerate(labels):
            got, rc = o.vcycle(src[:, j])
            err = float(np.linalg.norm(got - ref.ref[:, j]))
            assert rc == 0 and err <= tol[j], (cfg.label(), lab, err, tol[j])
            assert not got[K.zero_rows(name)].any()
            worst, S = max(worst, err / tol[j] if tol[j] > 0 else 0.0), max(S, ref.S)
    print(f"\n[mg] V-cycle {name}: S_case max {S:.2e}, coarse allowance {H.cg_allowance(K.VCYCLE_CONFIGS[0], TAU):.2e}, "
          f"oracle error / tolerance max {worst:.3f}")


def test_level0_is_the_lattice_the_device_forms():
    """the level 0 of A2, A3 and B3 is the constrained Q1 Laplacian of an nv^3 lattice, x fastest: what
    gmg_set_level_matrix_lattice forms from (nv, Ke), so that the four ways of the GPU test solve one operator"""
    for name in K.ADAPTIVE:
        H = K.hierarchy(name)[1]
        nv, Ke, lat = K.level0_lattice(name)
        csr, _ = so.assemble_constrained(lat, so.cell_matrices(lat), lat.boundary_mask())
        A0 = H.A[0]
        assert abs(R._scipy_csr(csr) - A0).max() <= 4 * R.U * abs(A0).max()


def test_layout_case_qualifies():
    """The library keeps a SELL-64 copy only of an operator with 1024 rows or more and a padding of at most 1.12; the layout
    switches change kernels for such operators alone.  Every operator of LAT's upper level qualifies (A_1, I_1, I_1^T, P_0,
    P_0^T), its level 0 does not (its CG sums in one order under every switch), and neither does any operator of the other
    hierarchies: on them a layout switch changes nothing, which is why the layout tests run on LAT."""
    def qualifies(m):
        rows, pad = K.sell_padding(m)
        return rows >= 1024 and pad <= 1.12

    h, H = K.hierarchy(K.LAT)
    ops = {"A1": H.A[1], "I1": H.I[1], "I1^T": H.I[1].T.tocsr(), "P0": H.P[1], "P0^T": H.P[1].T.tocsr()}
    for key, a in ops.items():
        a.sort_indices()
        rows, pad = K.sell_padding(K._csr_ns(a))
        print(f"\n[mg] LAT {key}: {rows} rows, SELL-64 padding {pad:.4f}")
        assert qualifies(K._csr_ns(a)), (key, rows, pad)
    assert not qualifies(K._csr_ns(H.A[0]))
    assert len(K.zero_rows(K.LAT)) == 8
    for name in K.NAMES:
        H = K.hierarchy(name)[1]
        for a in [m for m in H.A + H.I + H.P if m is not None]:
            assert not qualifies(K._csr_ns(a)) and not qualifies(K._csr_ns(a.T.tocsr())), name


def test_layout_case_oracle_and_sensitivity():
    """LAT as the GPU layout tests run it: the oracle against the reference, and every mutation that applies at 1000
    tolerances or more"""
    h, H = K.hierarchy(K.LAT)
    src, labels, dst0 = K.vcycle_sources(K.LAT)
    u0, rhs = K.smoother_vectors(K.LAT, 1)
    worst, S, low = 0.0, 0.0, {}
    for cfg in K.LAYOUT_CFGS:
        ref = K.vcycle_reference(K.LAT, cfg)
        tol = ref.tol + H.cg_allowance(cfg, TAU)
        o = oracle_mg(h, cfg)
        for j, lab in enumerate(labels):
            got, rc = o.vcycle(src[:, j])
            err = float(np.linalg.norm(got - ref.ref[:, j]))
            assert rc == 0 and err <= tol[j], (cfg.label(), lab, err, tol[j])
            assert not got[K.zero_rows(K.LAT)].any()
            worst, S = max(worst, err / tol[j]), max(S, ref.S)
        true = H.precondition("f64", cfg, src, dst0)
        for mut in vcycle_mutations(K.LAT, cfg):
            ratio = float((R.norm2(H.precondition("f64", cfg.with_mut(mut), src, dst0) - true) / tol).max())
            low[mut] = min(low.get(mut, np.inf), ratio)
            assert ratio >= R.SENSITIVITY, (cfg.label(), mut, ratio)
    for cfg in K.LAYOUT_SMOOTH:
        for from_zero in (True, False):
            ref = K.smoother_reference(K.LAT, 1, cfg, from_zero)
            err = float(np.linalg.norm(oracle_mg(h, cfg).smooth(1, u0, rhs, from_zero) - ref.ref))
            assert err <= ref.tol, (cfg.label(), from_zero, err, ref.tol)
            worst, S = max(worst, err / ref.tol), max(S, ref.S)
            true = H.smooth("f64", cfg, 1, u0, rhs, from_zero)
            for mut in smoother_mutations(cfg, from_zero):
                ratio = float(np.linalg.norm(H.smooth("f64", cfg.with_mut(mut), 1, u0, rhs, from_zero) - true)) / ref.tol
                low[mut] = min(low.get(mut, np.inf), ratio)
                assert ratio >= R.SENSITIVITY, (cfg.label(), from_zero, mut, ratio)
    print(f"\n[mg] LAT: S_case max {S:.2e}, oracle error / tolerance max {worst:.3f}; sensitivity (difference / tolerance, min): "
          + ", ".join(f"{m} {v:.1e}" for m, v in sorted(low.items())))


# ------------------------------------------------------------------------------------------------ the three evaluations of q

@pytest.mark.parametrize("degree", [1, 2, 3, 4])
@pytest.mark.parametrize("ratio,lmax", [(30.0, 0.0), (4.0, 0.0), (30.0, 1.7)])
def test_chebyshev_three_evaluations(degree, ratio, lmax):
    """Horner on the polynomial (f64), the product over the roots (ld) and the eigen-decomposition agree.  The bound is that
    of the two fp64 routes, not of the device: eigh returns eigenpairs to a few hundred u, and the monomial form cancels where
    the user's lmax lies below the spectrum's end (sum_j |c_j| x^j / |q(x)| reaches some hundreds at degree 4)"""
    H = K.hierarchy("A2")[1]
    cfg = R.Config(kind=R.CHEBYSHEV, degree=degree, ratio=ratio, lmax=lmax)
    r = K.smoother_vectors("A2", 1)[1][:, None]
    f, l = (H.levels(t)[1].chebyshev(cfg, r.astype(H.levels(t)[1].dtype)) for t in R.TIERS)
    e = R.chebyshev_by_eig(H.A[1], cfg, r)
    scale = float(np.linalg.norm(R.as_f64(l)))
    assert np.linalg.norm(f - R.as_f64(l)) <= 4096 * R.U * scale
    assert np.linalg.norm(e - R.as_f64(l)) <= 4096 * R.U * scale


def test_chebyshev_exchange_is_identity():
    """alpha and beta merely exchanged give the same polynomial (T_k(-x) = (-1)^k T_k(x) in numerator and denominator): that
    mutation cannot be seen by any test, which is why MUTATIONS carries the ratio on the wrong side instead"""
    from numpy.polynomial import chebyshev as C

    lam = np.linspace(0.01, 2.0, 97)
    for k in (1, 2, 3, 4):
        e = np.zeros(k + 1)
        e[-1] = 1.0
        p = [C.chebval((b + a - 2 * lam) / (b - a), e) / C.chebval((b + a) / (b - a), e) for a, b in ((0.06, 1.8), (1.8, 0.06))]
        assert np.abs(p[0] - p[1]).max() <= 16 * R.U * np.abs(p[0]).max()


# ------------------------------------------------------------------------------------------------ properties of the dense M

@pytest.mark.parametrize("name", ["A2", "A3", "B3", "SYN"])
def test_dense_M_properties(name):
    """With equal pre- and post-steps M is symmetric to rounding (bound: both M and M^T carry TOL_FACTOR S_case, S_case the
    tier spread of the same configuration), positive definite on the unconstrained DoFs, and its rows AND columns at the
    entries of no copy list (hanging nodes) are exactly 0.  Dirichlet DoFs are in the copy lists: their level rows are
    diag-only, so the smoothers and A_0^-1 act on them as scalars and M maps them to nonzero values, coupled to the free
    DoFs through the residual's columns -- the symmetric M includes them; the outer CG never sees them because its
    residual is 0 there.
    Cost: the dense M is formed for three smoothers x 1, 2, 3 steps; on B3 (2794 columns through the level-0 factorisation
    and the triangular solves, nine times) that is about 25 s of CPU time, on A3 about 15 s: the slowest tests of this file,
    accepted because the symmetry defects this pins were seen on exactly these hierarchies and step counts."""
    h, H = K.hierarchy(name)
    free = np.flatnonzero(~np.asarray(h.constrained, dtype=bool))
    zr = K.zero_rows(name)
    for cfg in [c for c in K.VCYCLE_CONFIGS if c.steps > 0]:   # without smoothing M is P A_0^-1 P^T: semi-definite only
        M = H.dense_M(cfg)
        S = K.vcycle_reference(name, cfg).S
        defect = float(np.linalg.norm(M - M.T) / np.linalg.norm(M))
        assert not M[zr].any() and not M[:, zr].any()
        ev = np.linalg.eigvalsh((M[np.ix_(free, free)] + M[np.ix_(free, free)].T) / 2)
        if name != "SYN":   # SYN's edge matrix is an arbitrary sparse matrix, not a mesh's: nothing makes its M symmetric
            assert defect <= 2 * R.TOL_FACTOR * S, (cfg.label(), defect, S)
            assert ev[0] > 0, (cfg.label(), ev[0])
        listed = np.setdiff1d(np.flatnonzero(np.asarray(h.constrained, dtype=bool)), zr)
        if len(listed):
            assert np.abs(M[listed, listed]).min() > 0
        print(f"\n[mg] M {name} {cfg.label()}: ||M - M^T|| / ||M|| = {defect:.2e} (bound {2 * R.TOL_FACTOR * S:.2e}), "
              f"lambda_min on the free DoFs {ev[0]:.3e}, kappa {ev[-1] / ev[0]:.1f}")


# ------------------------------------------------------------------------------------------------ sensitivity

def smoother_mutations(cfg, from_zero):
    if cfg.steps == 0:   # nothing runs: no mutation of a step can show
        return []
    out = ["one_step_fewer"]
    if from_zero:
        out.append("apply_not_from_zero")
    if cfg.kind == R.SSOR:
        out.append("ssor_omega_factor")
        if cfg.blocks > 1 and not cfg.bounds:
            out.append("ssor_coupled")
    if cfg.kind == R.CHEBYSHEV:
        out.append("cheb_interval")
    return out


def vcycle_mutations(name, cfg):
    H = K.hierarchy(name)[1]
    if cfg.steps == 0 and name == "hier3":
        # level 0 of hier3 is all boundary and the transfers carry no boundary column: without smoothing M is exactly 0
        # there (the device must return exact zeros, tolerance 0), and no mutation of the cycle can show
        return []
    out = ["skip_copy_entry"] + (["one_step_fewer"] if cfg.steps > 0 else [])
    if len(K.zero_rows(name)):   # hier3's copy lists cover every entry: nothing of dst survives them, zeroed or not
        out.append("no_zero_dst")
    if any(I is not None for I in H.I) and cfg.steps > 0:   # without smoothing u = 0 meets I, and nothing reads d after I^T
        out += ["drop_edge_out", "drop_edge_in", "edge_in_before_prolong"]
    if cfg.kind == R.SSOR and cfg.steps > 0:
        out.append("ssor_omega_factor")
    if cfg.kind == R.CHEBYSHEV:
        out.append("cheb_interval")
    return out


@pytest.mark.parametrize("name,level", K.SMOOTH_LEVELS)
def test_smoother_sensitivity(name, level):
    H = K.hierarchy(name)[1]
    u0, rhs = K.smoother_vectors(name, level)
    low = {}
    for cfg in K.smoother_configs(name, level):
        for from_zero in (True, False):
            ref = K.smoother_reference(name, level, cfg, from_zero)
            true = H.smooth("f64", cfg, level, u0, rhs, from_zero)
            for mut in smoother_mutations(cfg, from_zero):
                ratio = float(np.linalg.norm(H.smooth("f64", cfg.with_mut(mut), level, u0, rhs, from_zero) - true)) / ref.tol
                low[mut] = min(low.get(mut, np.inf), ratio)
                assert ratio >= R.SENSITIVITY, (cfg.label(), from_zero, mut, ratio)
    print(f"\n[mg] smoother sensitivity {name} level {level} (difference / tolerance, min over the cases): "
          + ", ".join(f"{m} {v:.1e}" for m, v in sorted(low.items())))


@pytest.mark.parametrize("name", K.NAMES)
def test_vcycle_sensitivity(name):
    """per (hierarchy, configuration, mutation): on at least one source the mutated M src differs from the true one by
    SENSITIVITY times that source's tolerance, the coarse allowance of tau = 1e-10 included"""
    H = K.hierarchy(name)[1]
    src, labels, dst0 = K.vcycle_sources(name)
    low = {}
    for cfg in K.VCYCLE_CONFIGS:
        ref = K.vcycle_reference(name, cfg)
        tol = ref.tol + H.cg_allowance(cfg, TAU)
        true = H.precondition("f64", cfg, src, dst0)
        for mut in vcycle_mutations(name, cfg):
            diff = R.norm2(H.precondition("f64", cfg.with_mut(mut), src, dst0) - true)
            ratio = float((diff / tol).max())
            low[mut] = min(low.get(mut, np.inf), ratio)
            assert ratio >= R.SENSITIVITY, (cfg.label(), mut, ratio)
    print(f"\n[mg] V-cycle sensitivity {name} (difference / tolerance, best source, min over the configurations): "
          + ", ".join(f"{m} {v:.1e}" for m, v in sorted(low.items())))


@pytest.mark.parametrize("name,level", K.RANK_SMOOTH_LEVELS)
def test_rank_smoother_sensitivity(name, level):
    """the SSOR partitions tests/test_gpu_ranks_reference.py sweeps on N ranks (B = N, 2 N, caller-given partitions with an empty
    and a one-row block): the same mutations at the same SENSITIVITY.  A partition whose reference decouples nothing (one block
    holds every row but one, or the level is too small for more than one block) cannot show ssor_coupled and is not asked to."""
    H = K.hierarchy(name)[1]
    u0, rhs = K.smoother_vectors(name, level)
    low = {}
    for cfg in K.rank_smoother_configs(name, level):
        for from_zero in (True, False):
            ref = K.smoother_reference(name, level, cfg, from_zero)
            true = H.smooth("f64", cfg, level, u0, rhs, from_zero)
            for mut in smoother_mutations(cfg, from_zero):
                ratio = float(np.linalg.norm(H.smooth("f64", cfg.with_mut(mut), level, u0, rhs, from_zero) - true)) / ref.tol
                low[mut] = min(low.get(mut, np.inf), ratio)
                assert ratio >= R.SENSITIVITY, (cfg.label(), from_zero, mut, ratio)
    print(f"\n[mg] rank smoother sensitivity {name} level {level} (difference / tolerance, min over the cases): "
          + ", ".join(f"{m} {v:.1e}" for m, v in sorted(low.items())))


@pytest.mark.parametrize("name", ["A3", "B3"])
def test_rank_vcycle_sensitivity(name):
    """the V-cycle with one SSOR block per rank (B = 2, 3): the oracle within tolerance and every mutation seen"""
    h, H = K.hierarchy(name)
    src, labels, dst0 = K.vcycle_sources(name)
    low, worst = {}, 0.0
    for cfg in K.RANK_VCYCLE_CONFIGS:
        ref = K.vcycle_reference(name, cfg)
        tol = ref.tol + H.cg_allowance(cfg, TAU)
        o = oracle_mg(h, cfg)
        for j, lab in enumerate(labels):
            got, rc = o.vcycle(src[:, j])
            err = float(np.linalg.norm(got - ref.ref[:, j]))
            assert rc == 0 and err <= tol[j], (cfg.label(), lab, err, tol[j])
            worst = max(worst, err / tol[j] if tol[j] > 0 else 0.0)
        true = H.precondition("f64", cfg, src, dst0)
        for mut in vcycle_mutations(name, cfg):
            ratio = float((R.norm2(H.precondition("f64", cfg.with_mut(mut), src, dst0) - true) / tol).max())
            low[mut] = min(low.get(mut, np.inf), ratio)
            assert ratio >= R.SENSITIVITY, (cfg.label(), mut, ratio)
    print(f"\n[mg] rank V-cycle {name}: oracle error / tolerance max {worst:.3f}; sensitivity (difference / tolerance, best source, min): "
          + ", ".join(f"{m} {v:.1e}" for m, v in sorted(low.items())))


# ------------------------------------------------------------------------------------------------ context reuse: twins and substitutions

REUSE_SOURCES = ("random", "random-free-x", "random-free-y")


def reuse_visible(name, cfg):
    """Without smoothing the cycle is u_1 = P A_0^-1 P^T d_1: u = 0 meets A_1 and I_1, and nothing reads d_1 after I_1^T (the
    reason vcycle_mutations gives for the edge mutations).  M then holds neither operator, no substitution of either can show,
    and the proof below asserts that instead: the two references are equal to the bit"""
    return cfg.steps > 0 or name not in ("SYN-A1", "SYN-I")


@pytest.mark.parametrize("name", K.REUSE_NAMES)
def test_reuse_case_discriminates(name):
    """tests/test_gpu_context_reuse.py loads SYN and then `name` into one context.  A context that kept
    a table derived from what `name` replaces computes SYN's M.  Per configuration and on each of the random source and the two
    random-free ones, SYN's M and `name`'s M are SENSITIVITY tolerances of `name` apart (the coarse allowance of tau = 1e-10
    included), so check_vcycle against `name`'s reference fails for such a context.  The sizes are SYN's: what the signature
    of the fused copies' tables holds is equal, and no stale index leaves its vector."""
    h, H = K.hierarchy(name)
    h0, H0 = K.hierarchy("SYN")
    assert H.n_sys == H0.n_sys and H.rows == H0.rows and [len(g) for g in H.copy_global] == [len(g) for g in H0.copy_global]
    src, labels, dst0 = K.vcycle_sources(name)
    cols = [labels.index(s) for s in REUSE_SOURCES]
    low = np.inf
    for cfg in K.VCYCLE_CONFIGS:
        ref = K.vcycle_reference(name, cfg)
        tol = (ref.tol + H.cg_allowance(cfg, TAU))[cols]
        other = H0.precondition("f64", cfg, src[:, cols], dst0)
        diff = R.norm2(other - ref.ref[:, cols])
        if not reuse_visible(name, cfg):
            assert np.array_equal(other, H.precondition("f64", cfg, src[:, cols], dst0)), cfg.label()   # (tier against the same tier)
            continue
        ratio = float((diff / tol).min())
        low = min(low, ratio)
        assert ratio >= R.SENSITIVITY, (cfg.label(), ratio)
    print(f"\n[mg] reuse {name} against SYN (difference / tolerance, worst of {', '.join(REUSE_SOURCES)}, min over the configurations): {low:.1e}")


def test_reuse_twin_stale_tables():
    """the defect itself, built explicitly: copy_to_mg and copy_from_mg through SYN's lists, everything else SYN-T's.  The
    operators are equal, so this is SYN's M (to the bit), and it is SENSITIVITY tolerances from SYN-T's M on SYN-T's sources"""
    from types import SimpleNamespace

    h, H = K.hierarchy(K.REUSE_TWIN)
    h0, H0 = K.hierarchy("SYN")
    assert not np.array_equal(np.sort(h.copy_global[1]), np.sort(h0.copy_global[1]))   # another assignment, not only another order
    assert not np.array_equal(np.sort(h.copy_global[0]), np.sort(h0.copy_global[0]))
    stale = SimpleNamespace(**vars(h))
    stale.copy_global, stale.copy_level = h0.copy_global, h0.copy_level
    Hs = R.Hierarchy(stale, "SYN-T with SYN's lists")
    src, labels, dst0 = K.vcycle_sources(K.REUSE_TWIN)
    cols = [labels.index(s) for s in REUSE_SOURCES]
    low = np.inf
    for cfg in K.VCYCLE_CONFIGS:
        ref = K.vcycle_reference(K.REUSE_TWIN, cfg)
        tol = (ref.tol + H.cg_allowance(cfg, TAU))[cols]
        got = Hs.precondition("f64", cfg, src[:, cols], dst0)
        assert np.array_equal(got, H0.precondition("f64", cfg, src[:, cols], dst0)), cfg.label()
        ratio = float((R.norm2(got - ref.ref[:, cols]) / tol).min())
        low = min(low, ratio)
        assert ratio >= R.SENSITIVITY, (cfg.label(), ratio)
    print(f"\n[mg] reuse SYN-T through SYN's copy tables (difference / tolerance, worst source, min over the configurations): {low:.1e}")


@pytest.mark.parametrize("name", ["SYN-A1", "SYN-I"])
def test_reuse_smoother_discriminates(name):
    """the smoother steps on level 1 that sequence 4 runs after each replacement: A_1's substitution is seen by every smoother
    with a step to run at SENSITIVITY tolerances; the edge matrix is no part of a smoother step (equal to the bit)"""
    H, H0 = K.hierarchy(name)[1], K.hierarchy("SYN")[1]
    u0, rhs = K.smoother_vectors(name, 1)
    low = np.inf
    for cfg in [c for c in K.VCYCLE_CONFIGS if c.steps > 0]:
        for from_zero in (True, False):
            ref = K.smoother_reference(name, 1, cfg, from_zero)
            diff = float(np.linalg.norm(H0.smooth("f64", cfg, 1, u0, rhs, from_zero) - ref.ref))
            if name == "SYN-I":
                assert diff <= ref.tol
                continue
            low = min(low, diff / ref.tol)
            assert diff / ref.tol >= R.SENSITIVITY, (cfg.label(), from_zero, diff / ref.tol)
    if name == "SYN-A1":
        print(f"\n[mg] reuse smoother SYN-A1 against SYN on level 1 (difference / tolerance, min): {low:.1e}")
