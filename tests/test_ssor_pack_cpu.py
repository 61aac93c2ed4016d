"""Rows of the SSOR sweep scheduled by slack (gmg_ssor_pack_levels, option sgs_pack; DESIGN.md 4 "Rows scheduled by slack"),
checked on the host against a restatement in plain Python -- the routines need neither a context nor a device.

The stages of a block are walked 32 rows at a time, so a stage of 40 rows costs two dependent steps.  The packed levels are a
list schedule of the same graph, restated here from its definition:
  height(i) = 0 if row i has no higher coupled neighbour, else 1 + max height(k) over its higher neighbours;
  step t = 0, 1, ...: a row is ready when all its lower coupled neighbours lie in steps < t; the step takes at most 32 ready
  rows, height descending, then row ascending;  level(i) = the row's step.
Checked: the level arrays are equal; every coupled lower neighbour lies in a lower level; no level holds more than 32 rows;
the level count lies between max(depth, ceil(coupled / 32)) and the stage-by-stage step count; the levels are the stages where
no stage exceeds 32 rows; the packed slot plan hands no slot to a new owner less than two steps after the old owner's last
reader (the check of tests/test_ssor_slots_cpu.py); the planner's records, replayed on the host by tests/ssor_plan_replay.cc,
give the sweep's values in both directions for matrices above the gate of 8192 rows."""
import functools

import numpy as np
import pytest

import ssor_plan_cases as spc
import ssor_shape_cases as K
from gpu_util import capi
from ssor_pack_cases import (MATRICES, ONE_BLOCK_ONLY, ROWS_PER_STEP, comb, comb_two_hubs, delayed_leaves, equal_runs, neighbours, restated, star,
                             wide_late_span)


def check_slots(m, rb, re, level, n_levels, backward):
    """the slot plan over the packed levels: steps = levels (backward: reversed), every reader later than what it reads, and
    per slot the next owner two steps behind the previous owner's last reader at the earliest"""
    step, last, slot, n_steps, n_slots = capi().ssor_slot_plan(m, rb, re, backward, packed=True)
    coupled = np.flatnonzero(level >= 0)
    want = np.where(level >= 0, n_levels - 1 - level if backward else level, -1)
    assert n_steps == n_levels and np.array_equal(step, want)
    lower, higher = neighbours(m, rb, re)
    rlast = step.copy()
    rp = m.rowptr
    for i in range(rb, re):   # readers by the stored entry a_ic alone: c < i forward, c > i backward
        for k in range(int(rp[i]), int(rp[i + 1])):
            c = int(m.col[k])
            if rb <= c < re and m.val[k] != 0 and (c > i if backward else c < i):
                assert step[i - rb] > step[c - rb] >= 0
                rlast[c - rb] = max(rlast[c - rb], step[i - rb])
    assert np.array_equal(last, rlast)
    assert np.array_equal(np.flatnonzero(slot >= 0), coupled)
    gap = 2
    for s in range(n_slots):
        owners = coupled[slot[coupled] == s]
        owners = owners[np.argsort(step[owners], kind="stable")]
        assert len(owners) > 0
        assert (step[owners[1:]] >= last[owners[:-1]] + gap).all()
        assert len(np.unique(step[owners])) == len(owners)
    assert slot.max(initial=-1) + 1 == n_slots
    if n_steps:
        live = np.zeros(n_steps + gap + 1, np.int64)
        np.add.at(live, step[coupled], 1)
        np.add.at(live, last[coupled] + gap, -1)
        assert np.cumsum(live).max() == n_slots
    return n_slots


def check_block(m, rb, re, slots=True):
    level, n_levels, stage_steps = capi().ssor_pack_levels(m, rb, re)
    rlevel, rn_levels, stage, rstage_steps = restated(m, rb, re)
    assert np.array_equal(level, rlevel) and n_levels == rn_levels and stage_steps == rstage_steps
    lower, _ = neighbours(m, rb, re)
    for i in range(re - rb):
        assert all(0 <= level[j] < level[i] for j in lower[i])
    coupled = level >= 0
    assert np.array_equal(coupled, stage >= 0)
    if coupled.any():
        assert np.bincount(level[coupled]).max() <= ROWS_PER_STEP
        depth = int(stage.max()) + 1
        assert max(depth, -(-int(coupled.sum()) // ROWS_PER_STEP)) <= n_levels <= stage_steps
        if np.bincount(stage[coupled]).max() <= ROWS_PER_STEP:
            assert np.array_equal(level, stage)
        # the stage-by-stage count is gmg_ssor_slot_plan's
        assert capi().ssor_slot_plan(m, rb, re, False)[3] == stage_steps
    else:
        assert n_levels == 0 and stage_steps == 0
    if slots:
        for backward in (False, True):
            check_slots(m, rb, re, level, n_levels, backward)
    return n_levels, stage_steps


# whole levels, and the thirds of a level as sub-blocks (the comb and the star have too few rows for three blocks)
@pytest.mark.parametrize("name,blocks", [(name, 1) for name in MATRICES] + [(name, 3) for name in MATRICES if name not in ONE_BLOCK_ONLY])
def test_levels_match_restatement(name, blocks):
    m = MATRICES[name]()
    br = equal_runs(m.n_rows, blocks)
    assert len(br) == blocks + 1
    for b in range(len(br) - 1):
        check_block(m, br[b], br[b + 1])


def test_comb_by_hand():
    m = comb()
    level, n_levels, stage_steps = capi().ssor_pack_levels(m, 0, 60)
    assert (n_levels, stage_steps) == (20, 21)   # the depth; the stages: row 1 and the 40 teeth are one stage of 41 rows
    assert level[:20].tolist() == list(range(20))
    assert np.flatnonzero(level == 1).tolist() == [1] + list(range(20, 51))
    assert np.flatnonzero(level == 2).tolist() == [2] + list(range(51, 60))
    # forward nobody reads a tooth; backward row 0 reads them all, so all 40 stay live to the last step
    assert check_slots(m, 0, 60, level, n_levels, True) >= 41


def test_comb_two_hubs_by_hand():
    m = comb_two_hubs()
    assert max(K.direction_entries(m)) == 19
    level, n_levels, stage_steps = capi().ssor_pack_levels(m, 0, 55)
    assert (n_levels, stage_steps) == (20, 21)
    assert level[:21].tolist() == list(range(20)) + [0]
    assert np.flatnonzero(level == 1).tolist() == [1] + list(range(21, 52))
    assert np.flatnonzero(level == 2).tolist() == [2] + list(range(52, 55))


def test_star_cannot_move():
    m = star()
    level, n_levels, stage_steps = capi().ssor_pack_levels(m, 0, 71)
    assert (n_levels, stage_steps) == (4, 4)
    assert level.tolist() == [0] + [1] * 32 + [2] * 32 + [3] * 6


def test_packed_levels_can_need_more_slots():
    """why the plan checks the packed levels against the y slots before it takes them: rows wait for delayed readers"""
    m = delayed_leaves()
    need = {packed: max(capi().ssor_slot_plan(m, 0, m.n_rows, backward, packed=packed)[4] for backward in (False, True)) for packed in (False, True)}
    assert need[True] >= 32 * 20 and need[False] <= 32 * 6, need


def test_bad_arguments_are_refused():
    import ctypes as C
    lib = capi().load()
    rp, col, val = np.array([0, 1, 2], np.int64), np.array([0, 1], np.int32), np.ones(2)
    p64, p32, pd = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    args = (rp.ctypes.data_as(p64), col.ctypes.data_as(p32), val.ctypes.data_as(pd))
    assert lib.gmg_ssor_pack_levels(C.c_int64(2), *args, C.c_int64(0), C.c_int64(3), None, None, None) == capi().ERR_INVALID
    assert lib.gmg_ssor_pack_levels(C.c_int64(2), args[0], args[1], None, C.c_int64(0), C.c_int64(2), None, None, None) == capi().ERR_INVALID
    assert lib.gmg_ssor_slot_plan_packed(C.c_int64(2), *args, C.c_int64(1), C.c_int64(0), C.c_int(0), None, None, None, None, None) == capi().ERR_INVALID
    nl, ns = C.c_int64(-1), C.c_int64(-1)
    assert lib.gmg_ssor_pack_levels(C.c_int64(2), *args, C.c_int64(0), C.c_int64(2), None, C.byref(nl), C.byref(ns)) == capi().OK
    assert (nl.value, ns.value) == (0, 0)  # two rows without couplings


# ---- the planner's records above the gate, replayed on the host ------------------------------------------------------------

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return K.build_replay(tmp_path_factory.mktemp("ssor_pack"))


REPLAYED = {"lattice27-21": lambda: spc.lattice27(21), "random-9000": lambda: spc.random_symmetric(n=9000)}


@functools.lru_cache(maxsize=None)
def replayed(name):
    return REPLAYED[name]()


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("name", list(REPLAYED))
def test_replay_of_packed_plans(exe, tmp_path, name, blocks):
    """the replay's option parser does not know sgs_pack: its default set packs by the gate (both matrices have more than 8192
    rows); the replay decodes every record and compares both directions with the sweep's definition"""
    m = replayed(name)
    assert m.n_rows >= 8192
    br = equal_runs(m.n_rows, blocks)
    packed = stages = 0
    for b in range(len(br) - 1):
        n_levels, stage_steps = check_block(m, br[b], br[b + 1], slots=False)
        packed += n_levels
        stages += stage_steps
    assert packed < stages
    K.write_case(tmp_path / "case", m, blocks, (), {"default": (), "sliding-off": (("sgs_sliding", 0),)})
    status, plans, _, err = K.replay(exe, tmp_path / "case")
    assert status == 0, err[-2000:]
    for plan in plans.values():
        assert plan["phased"] == 1 and plan["failures"] == 0
    assert plans["default"]["self_ranges"] == plans["default"]["ranges"] == 2 * blocks
    assert plans["default"]["steps"] == 2 * packed        # (both directions)
    assert plans["default"]["max_rows"] <= ROWS_PER_STEP
    assert plans["sliding-off"]["self_ranges"] == 0 and plans["sliding-off"]["steps"] == 2 * stages   # the ranged plan keeps the stages


def test_replay_keeps_the_stages_where_a_packed_step_has_no_shape(exe, tmp_path):
    """wide_late_span above the gate: packed, row 40 would come right after all 30 rows it reads and no shape holds 30 late
    columns; the block must be planned from its stages -- four waves, self-contained, the stage-by-stage steps -- and not
    handed to the one-wave sweep.  Below the gate the same plan."""
    plans = {}
    for n in (8191, 8200):
        m = wide_late_span(n)
        n_levels, stage_steps = check_block(m, 0, n, slots=False)
        assert (n_levels, stage_steps) == (3, 3)
        K.write_case(tmp_path / f"case{n}", m, 1, (), {"default": (), "sliding-off": (("sgs_sliding", 0),)})
        status, plans[n], _, err = K.replay(exe, tmp_path / f"case{n}")
        assert status == 0, err[-2000:]
        for plan in plans[n].values():
            assert (plan["phased"], plan["retried"], plan["failures"], plan["steps"]) == (1, 0, 0, 6), plan
        assert plans[n]["default"]["self_ranges"] == 2 and plans[n]["sliding-off"]["self_ranges"] == 0
    assert plans[8200] == plans[8191]
