"""Every record shape of the four-wave SSOR sweep on the MI355X (csrc/gmg_sgs_phase.hpp).  The matrices of
tests/ssor_shape_cases.py, each as level 1 of a synthetic two-level hierarchy:

  * the shape table rebuilt from the downloaded GMG_SSOR_PLAN_BLK_TAB and GMG_SSOR_PLAN_RANGES equals the one tests/ssor_plan_replay.cc
    prints for the same options on the CPU -- with the floor of tests/test_ssor_shapes_cpu.py this is the coverage assertion, read
    from what the kernel was launched with;
  * smoother_step with SSOR, omega = 0.5 and 0.8, 1 and 2 steps, from zero and from a given u, equals the oracle bit for bit (the
    bar of tests/test_gpu_ssor_sliding.py; for a caller-given partition the oracle is composed block by block as in
    tests/test_gpu_ssor_partition.py) and lies within mg_reference.tolerance(S_case, ref) of the longdouble tier of
    tests/mg_reference.py, S_case the spread of its two tiers: the definition by triangular solves, the rule and the constant 64
    of section 16;
  * the plan kinds sgs_sliding = 0, sgs_y_slots = 64, sgs_phase_chunk = 1 and the six SSOR_VARIANTS of tests/mg_cases.py give the
    default run's bits;
  * with ssor_plan_device the plan is built on the device and equals the host's byte for byte, or the origin gives the documented
    reason, which the test derives from the case (37 entries in a direction: "no shape");
  * two launches in a row are identical."""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import mg_cases
import mg_reference as R
import ssor_plan_cases as spc
import ssor_shape_cases as K
from gpu_util import capi
from oracle import gmg_oracle as go

pytestmark = pytest.mark.gpu
LEVEL = 1
CONFIGS = list(itertools.product((0.5, 0.8), (1, 2), (True, False)))   # omega, steps, from zero
CASE_NAMES = [c.name for c in K.CASES]
WORST = {}   # family -> worst error / tolerance seen (printed per family by the last test)


@functools.lru_cache(maxsize=None)
def setup(name):
    """(hierarchy, caller-given bounds or (), u0, rhs) of a case"""
    m, bounds = K.case(name).make()
    n = m.n_rows
    A0 = spc.tridiagonal(64)
    P = SimpleNamespace(n_rows=n, n_cols=64, nnz=n, rowptr=np.arange(n + 1, dtype=np.int64), col=(np.arange(n) % 64).astype(np.int32), val=np.ones(n))
    idx = np.arange(n, dtype=np.int32)
    empty = np.zeros(0, dtype=np.int32)
    hier = SimpleNamespace(system_matrix=m, level_matrices=[A0, m], edge_matrices=[None, None], prolongations=[P], copy_global=[empty, idx],
                           copy_level=[empty, idx])
    rng = np.random.default_rng(n)
    u0, rhs = rng.standard_normal(n), rng.standard_normal(n)
    for a in (u0, rhs):
        a.setflags(write=False)
    return hier, tuple(bounds), u0, rhs


def _diag_block(m, rb, re):
    """rows and columns [rb, re) of m as a matrix of its own"""
    rp, col, val = np.asarray(m.rowptr, np.int64), np.asarray(m.col, np.int64), np.asarray(m.val)
    rows = np.repeat(np.arange(rb, re), np.diff(rp[rb:re + 1]))
    c, v = col[rp[rb]:rp[re]], val[rp[rb]:rp[re]]
    keep = (c >= rb) & (c < re)
    rp_b = np.zeros(re - rb + 1, np.int64)
    np.cumsum(np.bincount(rows[keep] - rb, minlength=re - rb), out=rp_b[1:])
    return SimpleNamespace(n_rows=re - rb, n_cols=re - rb, nnz=int(keep.sum()), rowptr=rp_b, col=(c[keep] - rb).astype(np.int32), val=v[keep])


@functools.lru_cache(maxsize=None)
def oracle_steps(name):
    """the oracle's smoother step per configuration: computed once, read-only.  Equal runs: OracleMG.smooth; a caller-given
    partition: the oracle's SSOR block by block on the diagonal blocks, the residual steps on the whole matrix"""
    hier, bounds, u0, rhs = setup(name)
    A = hier.level_matrices[LEVEL]
    out = {}
    for omega, steps in {(o, s) for o, s, _ in CONFIGS}:
        if not bounds:
            mg = go.OracleMG(hier, smoother=go.SSOR, omega=omega, steps=steps, ssor_blocks=K.case(name).blocks)
            smooth = lambda u, from_zero: mg.smooth(LEVEL, u, rhs, from_zero)
        else:
            blocks = []
            for rb, re in zip(bounds, bounds[1:]):
                if re > rb:
                    Ab = _diag_block(A, rb, re)
                    h = SimpleNamespace(system_matrix=Ab, level_matrices=[Ab], edge_matrices=[None], prolongations=[], copy_global=[np.zeros(0, np.int32)],
                                        copy_level=[np.zeros(0, np.int32)])
                    blocks.append((rb, re, go.OracleMG(h, smoother=go.SSOR, omega=omega, steps=1)))

            def inverse(r):
                y = np.zeros(A.n_rows)
                for rb, re, mg in blocks:
                    y[rb:re] = mg.smooth(0, np.zeros(re - rb), r[rb:re], True)
                return y

            def smooth(u, from_zero, steps=steps, inverse=inverse):
                u = inverse(rhs) if from_zero else np.array(u)
                for _ in range(1 if from_zero else 0, steps):
                    u = u + inverse(rhs - go.spmv(A, u))
                return u
        for from_zero in (True, False):
            ref = smooth(u0, from_zero)
            ref.setflags(write=False)
            out[omega, steps, from_zero] = ref
    return out


@functools.lru_cache(maxsize=None)
def references(name):
    """per configuration (longdouble reference, tolerance): the definition by triangular solves, nothing from the library"""
    hier, bounds, u0, rhs = setup(name)
    H = R.Hierarchy(hier, name)
    out = {}
    for omega, steps, from_zero in CONFIGS:
        cfg = R.Config(kind=R.SSOR, omega=omega, steps=steps, blocks=K.case(name).blocks, bounds=((LEVEL, bounds),) if bounds else ())
        f64, ld = (H.smooth(tier, cfg, LEVEL, u0, rhs, from_zero) for tier in R.TIERS)
        out[omega, steps, from_zero] = (ld, float(R.tolerance(R.spread(f64, ld), ld)))
    return out


@functools.lru_cache(maxsize=None)
def cpu_plans(name):
    """what the replay says on the CPU, per option set: (plan numbers, shape table)"""
    import tempfile

    hier, bounds, _, _ = setup(name)
    with tempfile.TemporaryDirectory() as d:
        exe = _replay_exe()
        K.write_case(d + "/case", hier.level_matrices[LEVEL], K.case(name).blocks, bounds)
        status, plans, tables, err = K.replay(exe, d + "/case")
    assert status == 0, err
    return plans, tables


@functools.lru_cache(maxsize=None)
def _replay_exe():
    import tempfile

    _replay_exe.dir = tempfile.TemporaryDirectory()   # (kept alive with the function)
    return K.build_replay(_replay_exe.dir.name)


def context(name, options=(), device=False):
    hier, bounds, _, _ = setup(name)
    c = capi().Context(2)
    c.set_tuning(ssor_blocks=K.case(name).blocks)
    for key, value in options:
        c.set_option(key, value)
    if device:
        c.set_option("ssor_plan_device", 1)
    if bounds:
        c.set_ssor_block_rows(LEVEL, list(bounds))
    c.load_hierarchy(hier)
    return c


def step(c, name, omega, steps, from_zero):
    _, _, u0, rhs = setup(name)
    c.set_smoother(capi().SSOR, omega, steps)
    u, r = c.vector(len(u0), u0), c.vector(len(rhs), rhs)
    c.smoother_step(LEVEL, u, r, from_zero)
    out = u.download()
    u.free()
    r.free()
    return out


def device_table(c):
    """the shape table from the plan arrays of the context; None: the level has no four-wave plan"""
    A = capi()
    try:
        return K.table_from_arrays(c.get_ssor_plan_array(LEVEL, "ranges").tobytes(), c.get_ssor_plan_array(LEVEL, "blk_tab").tobytes())
    except A.GMGError as e:
        assert e.code == A.ERR_INVALID
        return None


def assert_table(c, name, option_set):
    plans, tables = cpu_plans(name)
    got = device_table(c)
    if plans[option_set]["phased"]:
        assert got == tables[option_set], (name, option_set)
    else:
        assert got is None, (name, option_set)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_default_plan_oracle_bits_and_reference(name):
    c = context(name)
    assert_table(c, name, "default")
    assert set(K.case(name).pairs) <= K.pairs_of(device_table(c) or {})
    worst = 0.0
    for cfg in CONFIGS:
        got = step(c, name, *cfg)
        ref, tol = references(name)[cfg]
        err = float(R.norm2(got.astype(np.longdouble) - ref))
        print(f"[ssor-shapes] {name} omega {cfg[0]} steps {cfg[1]} from_zero {cfg[2]}: error {err:.3e} tolerance {tol:.3e} ratio {err / tol:.3f}")
        worst = max(worst, err / tol)
        assert np.array_equal(got, oracle_steps(name)[cfg]), (name, cfg, float(np.abs(got - oracle_steps(name)[cfg]).max()))
        assert err <= tol, (name, cfg, err, tol)
        assert np.array_equal(step(c, name, *cfg), got), (name, cfg)   # two launches in a row
    c.close()
    family = K.case(name).family
    WORST[family] = max(WORST.get(family, 0.0), worst)


@pytest.mark.parametrize("kind", K.GPU_PLAN_KINDS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_plan_kinds_give_the_default_bits(name, kind):
    default = context(name)
    c = context(name, K.OPTION_SETS[kind])
    assert_table(c, name, kind)
    for cfg in CONFIGS:
        want = step(default, name, *cfg)
        assert np.array_equal(want, oracle_steps(name)[cfg]), (name, cfg)
        assert np.array_equal(step(c, name, *cfg), want), (name, kind, cfg)
    c.close()
    default.close()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_sweep_variants_give_the_default_bits(name):
    default = context(name)
    want = {cfg: step(default, name, *cfg) for cfg in CONFIGS}
    default.close()
    for variant, options in mg_cases.SSOR_VARIANTS.items():
        c = context(name, options)
        if variant in ("sgs_reg", "sgs_dep"):   # the field-major record layouts at this case's l1 / l2 (where the planner keeps the four waves)
            assert_table(c, name, variant[4:])
        for cfg in CONFIGS:
            assert np.array_equal(step(c, name, *cfg), want[cfg]), (name, variant, cfg)
        c.close()


def plan_arrays(c):
    A = capi()
    try:
        return {w: c.get_ssor_plan_array(LEVEL, w).tobytes() for w in A.SSOR_PLAN_ARRAYS}
    except A.GMGError as e:
        assert e.code == A.ERR_INVALID
        return None


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_builder_agrees_or_says_why(name):
    """the reason is derived from the case, not from the library's answer: a row with more than 36 entries in a direction has no
    shape; nothing else here keeps the device builder from the default plan (columns ascend, no row has more than 72 stored
    entries, every block's live rows fit the default y slots)"""
    m, _ = K.case(name).make()
    expect = "no shape" if max(K.direction_entries(m)) > 36 else "device"
    host, dev = context(name), context(name, device=True)
    assert host.get_ssor_plan_origin(LEVEL) == (False, 0, "")
    on_device, moved, why = dev.get_ssor_plan_origin(LEVEL)
    assert ("device" if on_device else why) == expect and moved == 0, (name, on_device, why)
    ref, got = plan_arrays(host), plan_arrays(dev)
    assert (ref is None) == (got is None) == (expect != "device")
    for w in ref or ():
        assert got[w] == ref[w], (name, w, len(ref[w]), len(got[w]))
    assert dev.get_ssor_plan(LEVEL) == host.get_ssor_plan(LEVEL)
    assert dev.get_ssor_backward_rows(LEVEL).tolist() == host.get_ssor_backward_rows(LEVEL).tolist()
    for cfg in CONFIGS[:2] + CONFIGS[-2:]:   # (only after the plans compared equal)
        assert np.array_equal(step(dev, name, *cfg), oracle_steps(name)[cfg]), (name, cfg)
    host.close()
    dev.close()


def test_report_worst_ratio_per_family():
    """one line per family, as the other reference tests print theirs (filled by the tests above when they ran in this process)"""
    for family, worst in sorted(WORST.items()):
        print(f"\n[ssor-shapes] family {family}: error / tolerance max {worst:.3f}")
        assert worst <= 1.0
