"""Rows of the SSOR sweep scheduled by slack on the MI355X (option sgs_pack, DESIGN.md 4 "Rows scheduled by slack").  The sweep
runs the same kernel over a shorter record stream: a row's value does not depend on the step that computes it, so with
sgs_pack = 1 smoother_step (SSOR, omega = 0.5, 2 steps, from zero and from a start vector) must equal the oracle bit for bit,
equal the same context with sgs_pack = 0, and repeat itself; gmg_get_ssor_schedule must report the counts that
tests/ssor_pack_cases.py restates from the definition.  Each matrix is level 1 of a synthetic two-level hierarchy, swept as
one block, as three, and under a caller-given partition with an empty block."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import ssor_plan_cases as spc
import ssor_shape_cases as K
from gpu_util import capi
from oracle import gmg_oracle as go
from ssor_pack_cases import MATRICES, comb, equal_runs, restated
from ssor_pack_cases import diag_block as _diag_block

pytestmark = pytest.mark.gpu
LEVEL = 1
OMEGA, STEPS = 0.5, 2
NAMES = ("comb", "comb-two-hubs", "lattice27-17", "random-3000", "A3-level1", "A3-level2", "B3-level1", "B3-level2")
PARTITIONS = ("B1", "B3", "given")
RUNS = [(name, part) for name in NAMES for part in PARTITIONS if not name.startswith("comb") or part == "B1"]   # (60 rows: one block)


@functools.lru_cache(maxsize=None)
def matrix(name):
    return spc.lattice27(21) if name == "lattice27-21" else MATRICES[name]()


@functools.lru_cache(maxsize=None)
def setup(name):
    """(hierarchy, u0, rhs): the matrix as level 1 over a small coarse level"""
    m = matrix(name)
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
    return hier, u0, rhs


def partition(name, part):
    """(blocks for gmg_set_ssor_blocks, caller-given bounds or (), the boundaries the plan uses)"""
    n = matrix(name).n_rows
    if part == "given":
        bounds = spc.given_bounds(n)
        return len(bounds) - 1, bounds, list(bounds)
    blocks = int(part[1:])
    return blocks, (), equal_runs(n, blocks)


@functools.lru_cache(maxsize=None)
def oracle_steps(name, part):
    """the oracle's smoother step, from zero and from u0: computed once, read-only (equal runs: OracleMG.smooth; a caller-given
    partition: the oracle's SSOR block by block on the diagonal blocks, as tests/test_gpu_ssor_shapes.py forms it)"""
    hier, u0, rhs = setup(name)
    A = hier.level_matrices[LEVEL]
    blocks, bounds, _ = partition(name, part)
    if not bounds:
        mg = go.OracleMG(hier, smoother=go.SSOR, omega=OMEGA, steps=STEPS, ssor_blocks=blocks)
        smooth = lambda u, from_zero: mg.smooth(LEVEL, u, rhs, from_zero)
    else:
        parts = []
        for rb, re in zip(bounds, bounds[1:]):
            if re > rb:
                Ab = _diag_block(A, rb, re)
                h = SimpleNamespace(system_matrix=Ab, level_matrices=[Ab], edge_matrices=[None], prolongations=[], copy_global=[np.zeros(0, np.int32)],
                                    copy_level=[np.zeros(0, np.int32)])
                parts.append((rb, re, go.OracleMG(h, smoother=go.SSOR, omega=OMEGA, steps=1)))

        def inverse(r):
            y = np.zeros(A.n_rows)
            for rb, re, mg in parts:
                y[rb:re] = mg.smooth(0, np.zeros(re - rb), r[rb:re], True)
            return y

        def smooth(u, from_zero):
            u = inverse(rhs) if from_zero else np.array(u)
            for _ in range(1 if from_zero else 0, STEPS):
                u = u + inverse(rhs - go.spmv(A, u))
            return u
    out = {}
    for from_zero in (True, False):
        out[from_zero] = smooth(u0, from_zero)
        out[from_zero].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated_counts(name, part):
    """(packed levels, stage-by-stage steps) of a direction, summed over the blocks"""
    _, _, br = partition(name, part)
    counts = [restated(matrix(name), rb, re)[1::2] for rb, re in zip(br, br[1:]) if re > rb]
    return sum(c[0] for c in counts), sum(c[1] for c in counts)


def context(name, part="B1", options=()):
    hier, _, _ = setup(name)
    blocks, bounds, _ = partition(name, part)
    c = capi().Context(2)
    c.set_tuning(ssor_blocks=blocks)
    for key, value in options:
        c.set_option(key, value)
    if bounds:
        c.set_ssor_block_rows(LEVEL, list(bounds))
    c.load_hierarchy(hier)
    return c


def step(c, name, from_zero):
    _, u0, rhs = setup(name)
    c.set_smoother(capi().SSOR, OMEGA, STEPS)
    u, r = c.vector(len(u0), u0), c.vector(len(rhs), rhs)
    c.smoother_step(LEVEL, u, r, from_zero)
    out = u.download()
    u.free()
    r.free()
    return out


@pytest.mark.parametrize("name,part", RUNS)
def test_packed_sweep_gives_the_oracle_bits(name, part):
    packed, stages = restated_counts(name, part)
    on, off = context(name, part, (("sgs_pack", 1),)), context(name, part, (("sgs_pack", 0),))
    plan = on.get_ssor_plan(LEVEL)
    # (derived from the matrix, not from the library's answer: a record of the four-wave sweep holds 36 entries of a direction; the
    # comb of 40 teeth has 42 in row 0 and is swept by the one-wave plan, which keeps the stages)
    if max(K.direction_entries(matrix(name))) <= 36:
        assert plan["self_contained_ranges"] == plan["forward_ranges"] + plan["backward_ranges"] > 0
        assert on.get_ssor_schedule(LEVEL) == {"packed": 1, "levels": packed, "steps_per_direction": packed, "stage_steps": stages}
        sched = off.get_ssor_schedule(LEVEL)
        assert (sched["packed"], sched["steps_per_direction"], sched["stage_steps"]) == (0, stages, stages)
        assert plan["steps"] == 2 * packed and off.get_ssor_plan(LEVEL)["steps"] == 2 * stages
    else:
        assert name == "comb" and plan["self_contained_ranges"] == 0 and on.get_ssor_schedule(LEVEL)["packed"] == 0
    for from_zero in (True, False):
        got = step(on, name, from_zero)
        want = oracle_steps(name, part)[from_zero]
        assert np.array_equal(got, want), (name, part, from_zero, float(np.abs(got - want).max()))
        assert np.array_equal(step(off, name, from_zero), got), (name, part, from_zero)
        assert np.array_equal(step(on, name, from_zero), got), (name, part, from_zero)   # applied twice in a row
    on.close()
    off.close()


def test_comb_moves_the_teeth():
    assert restated_counts("comb", "B1") == restated_counts("comb-two-hubs", "B1") == (20, 21)
    assert matrix("comb").n_rows == comb().n_rows == 60
    c = context("comb-two-hubs", "B1", (("sgs_pack", 1),))
    assert c.get_ssor_plan(LEVEL)["steps"] == 40   # 20 per direction: the depth
    c.close()


def test_stages_where_a_packed_step_has_no_shape():
    """wide_late_span of tests/ssor_pack_cases.py with sgs_pack = 1: packed, row 40 would have 30 late columns and no shape; the
    block keeps its stages and stays on the four-wave sweep with self-contained ranges -- the plan of sgs_pack = 0, array by array"""
    name = "wide-late-span"
    assert restated_counts(name, "B1") == (3, 3)
    on, off = context(name, "B1", (("sgs_pack", 1),)), context(name, "B1", (("sgs_pack", 0),))
    plan = on.get_ssor_plan(LEVEL)
    assert (plan["forward_ranges"], plan["backward_ranges"], plan["self_contained_ranges"], plan["steps"]) == (1, 1, 2, 6)
    assert on.get_ssor_schedule(LEVEL) == {"packed": 0, "levels": 2, "steps_per_direction": 3, "stage_steps": 3}
    for w in capi().SSOR_PLAN_ARRAYS:
        assert on.get_ssor_plan_array(LEVEL, w).tobytes() == off.get_ssor_plan_array(LEVEL, w).tobytes(), w
    for from_zero in (True, False):
        got = step(on, name, from_zero)
        assert np.array_equal(got, oracle_steps(name, "B1")[from_zero]), from_zero
        assert np.array_equal(step(off, name, from_zero), got), from_zero
    on.close()
    off.close()


def slots_needed(m, packed):
    """y slots (even) a block of the whole matrix needs as one range per direction: the larger direction's"""
    return max((capi().ssor_slot_plan(m, 0, m.n_rows, backward, packed=packed)[4] + 1) & ~1 for backward in (False, True))


def test_stages_where_the_packed_levels_do_not_fit():
    """an LDS budget of exactly the slots the stages need, fewer than the packed levels need (the matrix of
    tests/ssor_pack_cases.py whose leaves wait): the plan is the unpacked, self-contained one, and the bits are the same"""
    name = "delayed-leaves"
    m = matrix(name)
    y = slots_needed(m, False)
    assert 64 <= y < slots_needed(m, True), (y, slots_needed(m, True))
    _, stages = restated_counts(name, "B1")
    c = context(name, "B1", (("sgs_pack", 1), ("sgs_y_slots", y)))
    plan = c.get_ssor_plan(LEVEL)
    assert (plan["self_contained_ranges"], plan["y_slots"], plan["steps"]) == (2, y, 2 * stages)
    assert c.get_ssor_schedule(LEVEL) == {"packed": 0, "levels": 21, "steps_per_direction": stages, "stage_steps": stages}   # 21 stages: 20 deep, the last leaves
    roomy = context(name, "B1", (("sgs_pack", 1),))
    assert roomy.get_ssor_schedule(LEVEL)["packed"] == 1 and roomy.get_ssor_plan(LEVEL)["y_slots"] == slots_needed(m, True)
    for from_zero in (True, False):
        got = step(c, name, from_zero)
        assert np.array_equal(got, oracle_steps(name, "B1")[from_zero]), from_zero
        assert np.array_equal(step(roomy, name, from_zero), got), from_zero
    c.close()
    roomy.close()


@pytest.mark.parametrize("name,part", [("lattice27-17", "B1"), ("A3-level1", "B3"), ("random-3000", "given")])
def test_device_builder_leaves_packed_levels_to_the_host(name, part):
    host = context(name, part, (("sgs_pack", 1),))
    dev = context(name, part, (("sgs_pack", 1), ("ssor_plan_device", 1)))
    assert host.get_ssor_plan_origin(LEVEL) == (False, 0, "")
    assert dev.get_ssor_plan_origin(LEVEL) == (False, 0, "packed schedule")
    for w in capi().SSOR_PLAN_ARRAYS:
        assert dev.get_ssor_plan_array(LEVEL, w).tobytes() == host.get_ssor_plan_array(LEVEL, w).tobytes(), (name, part, w)
    assert dev.get_ssor_schedule(LEVEL) == host.get_ssor_schedule(LEVEL) and dev.get_ssor_schedule(LEVEL)["packed"] == 1
    # with sgs_pack = 0 the device builder plans as before
    plain = context(name, part, (("sgs_pack", 0), ("ssor_plan_device", 1)))
    assert plain.get_ssor_plan_origin(LEVEL) == (True, 0, "")
    assert plain.get_ssor_schedule(LEVEL)["packed"] == 0
    for c in (host, dev, plain):
        c.close()


def test_automatic_above_the_gate():
    """no option set: a level of 9261 rows is packed, one of 4913 rows is not"""
    name = "lattice27-21"
    packed, stages = restated_counts(name, "B1")
    assert matrix(name).n_rows >= 8192 and packed < stages
    c = context(name)
    assert c.get_ssor_schedule(LEVEL) == {"packed": 1, "levels": packed, "steps_per_direction": packed, "stage_steps": stages}
    for from_zero in (True, False):
        assert np.array_equal(step(c, name, from_zero), oracle_steps(name, "B1")[from_zero]), from_zero
    c.close()
    small = context("lattice27-17")
    assert small.get_ssor_schedule(LEVEL)["packed"] == 0
    small.close()
