"""The device's smoothers and V-cycle (smooth_level, cheb_apply, level_v_step, vcycle in csrc/gmg_coulomb.hip) through capi.Context
against tests/mg_reference.py, the definitions written as closed-form dense-style operators that share no text with the oracle
(DESIGN.md section 16).  Tolerance on a vector, in the 2-norm: 64 S_case ||ref||_2 + the coarse allowance; S_case is the spread of
the reference's own two tiers on that case and the allowance comes from lambda_min(A_0), kappa_2(A_0) and ||T||_2 of the reference.
tests/test_mg_reference_cpu.py proves that every mutation of the definition is 1000 tolerances or more away on these cases.
Each test prints its worst error / tolerance ("[mg-gpu]", run with -s)."""
import numpy as np
import pytest

import mg_cases as K
import mg_reference as R
from gpu_util import capi

pytestmark = pytest.mark.gpu

TAU = 1e-10


def load(c, h, lattice=None):
    """Context.load_hierarchy, with level 0 formed on the device from (nv, Ke) when lattice is given"""
    if lattice is None:
        c.load_hierarchy(h)
        return
    c.set_system_matrix(h.system_matrix)
    for l, A in enumerate(h.level_matrices):
        if l == 0:
            c.set_level_matrix_lattice(0, lattice[0], lattice[1])
        else:
            c.set_level_matrix(l, A)
        I = h.edge_matrices[l]
        if I is not None and I.nnz > 0:
            c.set_edge_matrix(l, I)
        c.set_copy_indices(l, h.copy_global[l], h.copy_level[l])
    for l, P in enumerate(h.prolongations):
        c.set_prolongation(l, P)


def context(name, options=(), blocks=0, level_rows=None, lattice=None):
    h = K.hierarchy(name)[0]
    c = capi().Context(len(h.level_matrices))
    if blocks:
        c.set_tuning(ssor_blocks=blocks)
    for key, value in options:
        c.set_option(key, value)
    for level, rows in (level_rows or {}).items():
        c.set_ssor_block_rows(level, list(rows))
    load(c, h, lattice)
    return c


def set_smoother(c, cfg):
    c.set_smoother(cfg.kind, cfg.omega, cfg.steps, cheb_degree=cfg.degree, cheb_ratio=cfg.ratio, cheb_lmax=cfg.lmax)


def smooth(c, level, u0, rhs, from_zero):
    u, r = c.vector(len(u0), u0), c.vector(len(rhs), rhs)
    c.smoother_step(level, u, r, from_zero)
    out = u.download()
    u.free()
    r.free()
    return out


def precondition(c, src, dst0):
    vs, vd = c.vector(len(src), src), c.vector(len(src), dst0)
    c.precondition(vd, vs)
    out = vd.download()
    vs.free()
    vd.free()
    return out


@pytest.fixture(scope="module")
def default_ctx():
    made = {}

    def get(name):
        if name not in made:
            made[name] = context(name)
        return made[name]

    yield get
    for c in made.values():
        c.close()


# ------------------------------------------------------------------------------------------------ smoother_step

@pytest.mark.parametrize("name,level", K.SMOOTH_LEVELS)
def test_smoother_step(default_ctx, name, level):
    """Jacobi, SSOR (B = 1, 3 and a caller-given partition with an empty and a one-row block) and Chebyshev (degree 1-4,
    ratio 30 and 4, a user lmax) with 1, 2 and 3 steps, apply and smooth"""
    u0, rhs = K.smoother_vectors(name, level)
    n = len(u0)
    ctxs = {1: default_ctx(name), 3: context(name, blocks=3), "given": context(name, level_rows={level: K.given_bounds(n)})}
    worst = {}
    for cfg in K.smoother_configs(name, level):
        c = ctxs["given" if cfg.bounds else cfg.blocks]
        set_smoother(c, cfg)
        for from_zero in (True, False):
            ref = K.smoother_reference(name, level, cfg, from_zero)
            err = float(np.linalg.norm(smooth(c, level, u0, rhs, from_zero) - ref.ref))
            kind = R.KIND_NAMES[cfg.kind]
            worst[kind] = max(worst.get(kind, 0.0), err / ref.tol)
            assert err <= ref.tol, (cfg.label(), from_zero, err, ref.tol, ref.S)
    ctxs[3].close()
    ctxs["given"].close()
    print(f"\n[mg-gpu] smoother_step {name} level {level}: error / tolerance max " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("variant", list(K.SSOR_VARIANTS))
@pytest.mark.parametrize("name", ["A3", "B3"])
def test_ssor_variants(name, variant):
    """every SSOR sweep kernel, B = 1 and 3, on both upper levels with 1, 2 and 3 steps"""
    H = K.hierarchy(name)[1]
    worst = 0.0
    for blocks in (1, 3):
        c = context(name, options=K.SSOR_VARIANTS[variant], blocks=blocks)
        for level in range(1, H.n_levels):
            u0, rhs = K.smoother_vectors(name, level)
            for steps in (1, 2, 3):
                cfg = R.Config(kind=R.SSOR, steps=steps, blocks=blocks)
                set_smoother(c, cfg)
                for from_zero in (True, False):
                    ref = K.smoother_reference(name, level, cfg, from_zero)
                    err = float(np.linalg.norm(smooth(c, level, u0, rhs, from_zero) - ref.ref))
                    worst = max(worst, err / ref.tol)
                    assert err <= ref.tol, (level, cfg.label(), from_zero, err, ref.tol)
        c.close()
    print(f"\n[mg-gpu] SSOR {variant} {name}: error / tolerance max {worst:.3f}")


# ------------------------------------------------------------------------------------------------ precondition

def check_vcycle(name, cfg, got, allowance, what):
    """got [n_sys, k] against the reference: within tolerance, exact zeros where M's rows are exactly zero, and
    <y, M x> = <x, M y> for the pair of sources with the constrained entries zeroed.  The symmetry bound: got_x = M x + e_x
    with ||e_x|| <= tol_x, so |<y, got_x> - <x, got_y>| <= |<y, M x> - <x, M y>| + ||y|| tol_x + ||x|| tol_y, the first term
    taken from the reference's longdouble tier.  This is the bound of tests/test_mg_reference_cpu.py (M and M^T each carry
    TOL_FACTOR S_case) written per source, with the coarse allowance added.  It follows from the error assertions above it
    and cannot fail on its own: it is kept as the statement that a device result within tolerance is symmetric to this
    accuracy, and the symmetry of M itself is what test_dense_M_properties asserts on the reference."""
    ref = K.vcycle_reference(name, cfg)
    src, labels, dst0 = K.vcycle_sources(name)
    tol = ref.tol + allowance
    err = R.norm2(got - ref.ref)
    for j, lab in enumerate(labels):
        assert err[j] <= tol[j], (what, cfg.label(), lab, err[j], tol[j], ref.S)
    assert not got[K.zero_rows(name)].any(), (what, cfg.label())
    ld = np.longdouble
    ix, iy = labels.index("random-free-x"), labels.index("random-free-y")
    x, y = src[:, ix].astype(ld), src[:, iy].astype(ld)
    defect = abs(float(y @ got[:, ix].astype(ld) - x @ got[:, iy].astype(ld)))
    own = abs(float(y @ ref.ld[:, ix] - x @ ref.ld[:, iy]))
    bound = own + float(np.linalg.norm(src[:, iy])) * tol[ix] + float(np.linalg.norm(src[:, ix])) * tol[iy]
    assert defect <= bound, (what, cfg.label(), defect, bound)
    plain = float(np.max(err / np.where(ref.tol > 0, ref.tol, np.inf)))
    return float(np.max(err / np.where(tol > 0, tol, np.inf))), plain, (defect / bound if bound > 0 else 0.0)


def run_sources(c, name):
    src, labels, dst0 = K.vcycle_sources(name)
    return np.stack([precondition(c, src[:, j], dst0) for j in range(src.shape[1])], axis=1)


@pytest.mark.parametrize("name", K.NAMES)
def test_precondition(default_ctx, name):
    """gmg_precondition with the coarse CG at its default tau = 1e-10: three smoothers x 1, 2, 3 steps x all sources; dst
    holds other values before every call"""
    H = K.hierarchy(name)[1]
    c = default_ctx(name)
    c.set_coarse(TAU, 1000)
    worst = [0.0, 0.0, 0.0]
    for cfg in K.VCYCLE_CONFIGS:
        set_smoother(c, cfg)
        r = check_vcycle(name, cfg, run_sources(c, name), H.cg_allowance(cfg, TAU), "cg")
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"\n[mg-gpu] precondition {name}: error / tolerance max {worst[0]:.3f} (without the coarse allowance {worst[1]:.3g}), "
          f"symmetry defect / bound max {worst[2]:.3f}")


@pytest.mark.parametrize("name", ["A2", "A3", "B3"])
def test_level0_four_ways(name):
    """level 0 as a CSR with the coarse CG at tau = 1e-10 and at the tau the reference's kappa_2(A_0) says the CG can reach
    (64 u kappa_2 ||d_0||, set per source); formed by gmg_set_level_matrix_lattice with the CG and with the direct solver"""
    C = capi()
    h, H = K.hierarchy(name)
    src, labels, dst0 = K.vcycle_sources(name)
    shape, Ke, _ = K.level0_lattice(name)
    cfgs = [R.Config(kind=R.SSOR, steps=2), R.Config(kind=R.JACOBI, steps=3, degree=3)]
    assert all(cfg in K.VCYCLE_CONFIGS for cfg in cfgs)
    out = {}
    for way in ("csr-cg", "csr-cg-tight", "lattice-cg", "lattice-direct"):
        c = context(name, lattice=(shape, Ke) if way.startswith("lattice") else None)
        if way == "lattice-direct":
            c.set_coarse_solver(C.COARSE_DIRECT)
        for cfg in cfgs:
            ref = K.vcycle_reference(name, cfg)
            set_smoother(c, cfg)
            if way == "csr-cg-tight":
                tau = H.cg_floor() * np.where(ref.d0_norm > 0, ref.d0_norm, 1.0)
                cols = []
                for j in range(src.shape[1]):
                    c.set_coarse(float(tau[j]), 1000)
                    cols.append(precondition(c, src[:, j], dst0))
                got, allowance = np.stack(cols, axis=1), tau / H.coarse_spectrum[0] * H.coarse_map_norm(cfg)
            else:
                c.set_coarse(TAU, 1000)
                got = run_sources(c, name)
                allowance = H.direct_allowance(cfg, shape, ref.coarse_norm) if way == "lattice-direct" else H.cg_allowance(cfg, TAU)
            r = check_vcycle(name, cfg, got, allowance, way)
            out[way] = max(out.get(way, 0.0), r[0])
        st = c.stats()
        assert int(st.coarse_solver) == (C.COARSE_DIRECT if way == "lattice-direct" else C.COARSE_CG)
        assert bool(int(st.spmv0_layout) & 64) == way.startswith("lattice")
        c.close()
    print(f"\n[mg-gpu] level 0 four ways {name}: error / tolerance max " + ", ".join(f"{k} {v:.3g}" for k, v in out.items()))


# ------------------------------------------------------------------------------------------------ layouts

ALL_LAYOUTS = 1 + 2 + 4 + 8 + 16 + 32


def probe_layout(matrix, options):
    """gmg_stats reports the layout of level 0 alone, so the layout an upper-level operator gets under these options is read
    from a one-level context that holds it as its level 0: the same gmg_set_level_matrix, the same decision"""
    c = capi().Context(1)
    for key, value in options:
        c.set_option(key, value)
    c.set_level_matrix(0, matrix)
    lay = int(c.stats().spmv0_layout)
    c.close()
    return lay


def layout_run(c):
    H = K.hierarchy(K.LAT)[1]
    out = {}
    c.set_coarse(TAU, 1000)
    for cfg in K.LAYOUT_CFGS:
        set_smoother(c, cfg)
        out["v", cfg] = run_sources(c, K.LAT)
    u0, rhs = K.smoother_vectors(K.LAT, 1)
    for cfg in K.LAYOUT_SMOOTH:
        set_smoother(c, cfg)
        for from_zero in (True, False):
            out["s", cfg, from_zero] = smooth(c, 1, u0, rhs, from_zero)
    return out


@pytest.fixture(scope="module")
def layout_default():
    """the default run of LAT, checked against the reference once, and the layouts its operators have by default"""
    h, H = K.hierarchy(K.LAT)
    c = context(K.LAT)
    base = layout_run(c)
    lay_level0 = int(c.stats().spmv0_layout)
    c.close()
    worst = 0.0
    for key, val in base.items():
        if key[0] == "s":
            ref = K.smoother_reference(K.LAT, 1, key[1], key[2])
            err = float(np.linalg.norm(val - ref.ref))
            assert err <= ref.tol, (key[1].label(), key[2], err, ref.tol)
            worst = max(worst, err / ref.tol)
        else:
            worst = max(worst, check_vcycle(K.LAT, key[1], val, H.cg_allowance(key[1], TAU), "default")[0])
    lay_A, lay_I = probe_layout(h.level_matrices[1], ()), probe_layout(h.edge_matrices[1], ())
    print(f"\n[mg-gpu] layouts LAT default: error / tolerance max {worst:.3f}, layout of A_1 {lay_A}, of I_1 {lay_I}, of A_0 {lay_level0}")
    # the level operator has every layout there is; the edge matrix is a SELL-64 copy; level 0 stays on CSR row windows
    assert lay_A == ALL_LAYOUTS and lay_I & 1 and lay_level0 == 0
    return base, lay_A, lay_I


@pytest.mark.parametrize("switch", K.LAYOUT_SWITCHES)
def test_layouts(layout_default, switch):
    """The V-cycle and the smoother steps on LAT, whose level operator, edge matrix, prolongation and their transposes all
    qualify for the SELL-64 layouts (tests/test_mg_reference_cpu.py: test_layout_case_qualifies), with each diagnostic switch
    that changes which SpMV kernel serves them: the residual, add-to, Jacobi and Chebyshev epilogues on the CSR row-window
    kernel, on spmv_sell_kernel with and without column patterns, value codes and 16-bit columns, on spmv_sellp_kernel with
    and without row classes, and the plain product on the lattice kernel.  The default run has every layout bit set and the
    switch must clear its bits.  A row is summed in its stored order in every layout and level 0 (CSR under every switch) runs
    the same CG, so every result is the default run's bits, and the default run is within tolerance of the reference."""
    h, H = K.hierarchy(K.LAT)
    base, lay_A, lay_I = layout_default
    options = ((switch, 1),)
    lay = probe_layout(h.level_matrices[1], options)
    assert lay_A & K.LAYOUT_CLEARS[switch] == K.LAYOUT_CLEARS[switch]
    assert lay == lay_A & ~K.LAYOUT_CLEARS[switch], (switch, lay_A, lay)
    if switch == "disable_sell":
        assert probe_layout(h.edge_matrices[1], options) == 0
    c = context(K.LAT, options=options)
    got = layout_run(c)
    c.close()
    differ = []
    for key, val in got.items():
        if key[0] == "s":
            ref = K.smoother_reference(K.LAT, 1, key[1], key[2])
            assert float(np.linalg.norm(val - ref.ref)) <= ref.tol, (switch, key[1].label(), key[2])
        else:
            check_vcycle(K.LAT, key[1], val, H.cg_allowance(key[1], TAU), switch)
        if not np.array_equal(val, base[key]):
            differ.append((key[0], key[1].label(), float(np.abs(val - base[key]).max())))
    print(f"\n[mg-gpu] layouts LAT {switch}: layout of A_1 {lay_A} -> {lay}, {len(got) - len(differ)} of {len(got)} results are the default's bits")
    assert not differ, (switch, differ)


# ------------------------------------------------------------------------------------------------ state across calls

def test_state_across_calls():
    """the Jacobi steps run out of place and leave a level's sol / w1 exchanged after an odd count; nothing of that may
    reach the next call"""
    name = "A3"
    h, H = K.hierarchy(name)
    src, labels, dst0 = K.vcycle_sources(name)
    x = src[:, 0]
    J1, J3 = R.Config(kind=R.JACOBI, steps=1, degree=3), R.Config(kind=R.JACOBI, steps=3, degree=3)
    S2, C2 = R.Config(kind=R.SSOR, steps=2), R.Config(kind=R.CHEBYSHEV, steps=2, degree=2)

    def fresh(cfg):
        c = context(name)
        set_smoother(c, cfg)
        out = precondition(c, x, dst0)
        c.close()
        return out

    expect = {cfg: fresh(cfg) for cfg in (J1, J3, S2, C2)}
    c = context(name)
    for cfg in (J1, J3):                      # the same V-cycle twice: identical bits
        set_smoother(c, cfg)
        a, b = precondition(c, x, dst0), precondition(c, x, np.zeros_like(dst0))
        assert np.array_equal(a, b) and np.array_equal(a, expect[cfg]), cfg.label()
    for cfg in (J3, S2, C2, J3):              # a chain without reloading: each equals a fresh context's bits
        set_smoother(c, cfg)
        assert np.array_equal(precondition(c, x, dst0), expect[cfg]), cfg.label()
    set_smoother(c, J3)                       # smoother_step between two V-cycles does not change the second
    a = precondition(c, x, dst0)
    for level in (1, 2):
        u0, rhs = K.smoother_vectors(name, level)
        smooth(c, level, u0, rhs, False)
        smooth(c, level, u0, rhs, True)
    assert np.array_equal(precondition(c, x, dst0), a)
    n = H.n_sys                               # a solve after all of that: the iteration count of a fresh context
    vb, vx = c.vector(n, h.system_rhs), c.vector(n)
    after = c.cg_solve(vx, vb)
    xa = vx.download()
    vb.free()
    vx.free()
    c.close()
    c = context(name)
    set_smoother(c, J3)
    vb, vx = c.vector(n, h.system_rhs), c.vector(n)
    first = c.cg_solve(vx, vb)
    xf = vx.download()
    vb.free()
    vx.free()
    c.close()
    assert after["status"] == first["status"] == 0 and after["iterations"] == first["iterations"]
    assert np.array_equal(xa, xf)
