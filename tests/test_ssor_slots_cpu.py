"""The y slots of the SSOR sweep's self-contained ranges (gmg_ssor_slot_plan, DESIGN.md 4 "One range per direction"),
checked on the host against a numpy restatement -- the routine needs neither a context nor a device.

A whole sweep direction of a block is one LDS range when the rows that are LIVE, not all rows it touches, fit the y
slots: a row owns a slot from the step that updates it to the step of its last reader, then the slot changes hands.
What the kernel relies on, and what is checked here:
  * a reader's step is later than the step of every column it reads (the value is there);
  * rows whose intervals [step, last reader] overlap never share a slot;
  * a slot's next owner comes two steps after the previous owner's last reader at the earliest: a step touches its
    rows' slots one phase before its dependent phase already, while the step before it may still read or write;
  * the lowest free slot is always taken, so the slot count is the most slots ever live and is deterministic."""
import heapq

import numpy as np
import pytest

from gpu_util import capi
from oracle import step50_oracle as so

ROWS_PER_STEP = 32


def restated_plan(m, rb, re, backward):
    """(step, last_reader, slot, n_steps, n_slots, readers) of rows [rb, re), restated.  Entries: stored value != 0, column in
    the block.  stage(i) = 1 + max stage(j) over the j in [rb, i) coupled to i through a_ij or a_ji.  Steps: the stages
    ascending (backward: descending), <= 32 rows of a stage per step, rows ascending (backward: descending).  A row's
    readers: rows i with an entry a_ic, c < i (backward: c > i).  Slots: before a step's rows are placed, the slots of the
    rows with last reader < s - 1 are freed; every row takes the lowest free slot."""
    rp, col, val = np.asarray(m.rowptr, np.int64), np.asarray(m.col, np.int64), np.asarray(m.val)
    nb = re - rb
    r = np.repeat(np.arange(rb, re), np.diff(rp[rb:re + 1])) - rb
    c, v = col[rp[rb]:rp[re]] - rb, val[rp[rb]:rp[re]]
    keep = (c >= 0) & (c < nb) & (v != 0)
    r, c = r[keep], c[keep]
    off = r != c
    lo, hi = np.minimum(r[off], c[off]), np.maximum(r[off], c[off])
    coupled = np.zeros(nb, bool)
    coupled[lo] = True
    coupled[hi] = True
    order = np.argsort(hi, kind="stable")
    lo_s, hi_s = lo[order], hi[order]
    starts = np.searchsorted(hi_s, np.arange(nb + 1))
    stage = np.zeros(nb, np.int64)
    for i in range(nb):
        if starts[i + 1] > starts[i]:
            stage[i] = stage[lo_s[starts[i]:starts[i + 1]]].max() + 1
    step = np.full(nb, -1, np.int64)
    rows_of_step = []
    n_stages = int(stage[coupled].max()) + 1 if coupled.any() else 0
    for t in (range(n_stages - 1, -1, -1) if backward else range(n_stages)):
        rows = np.flatnonzero(coupled & (stage == t))
        if backward:
            rows = rows[::-1]
        for k in range(0, len(rows), ROWS_PER_STEP):
            step[rows[k:k + ROWS_PER_STEP]] = len(rows_of_step)
            rows_of_step.append(rows[k:k + ROWS_PER_STEP])
    reads = (c > r) if backward else (c < r)  # entry (r, c): row r gathers column c in this direction
    readers = (r[reads], c[reads])
    last = step.copy()
    np.maximum.at(last, readers[1], step[readers[0]])
    hold = 2
    slot = np.full(nb, -1, np.int64)
    due = [[] for _ in range(len(rows_of_step) + 1)]
    free, n_slots = [], 0
    for s, rows in enumerate(rows_of_step):
        for i in due[s]:
            heapq.heappush(free, int(slot[i]))
        for i in rows:
            if free:
                slot[i] = heapq.heappop(free)
            else:
                slot[i] = n_slots
                n_slots += 1
            if last[i] + hold < len(rows_of_step):
                due[last[i] + hold].append(i)
    return step, last, slot, len(rows_of_step), n_slots, readers


def check_block(m, rb, re, backward):
    step, last, slot, n_steps, n_slots = capi().ssor_slot_plan(m, rb, re, backward)
    rstep, rlast, rslot, rn_steps, rn_slots, (rd_row, rd_col) = restated_plan(m, rb, re, backward)
    assert np.array_equal(step, rstep) and n_steps == rn_steps  # steps agree
    assert np.array_equal(last, rlast)
    # every reader's step is later than the step of each column it reads
    assert (step[rd_row] > step[rd_col]).all() and (step[rd_col] >= 0).all()
    assert (last >= step).all()
    # every coupled row of the block has a step and a slot, no other row has (what the backward RECORDS carry as the row to
    # store to: tests/ssor_plan_replay.cc decodes the plan's records on the host)
    coupled = np.flatnonzero(rstep >= 0)
    assert np.array_equal(np.flatnonzero(step >= 0), coupled) and np.array_equal(np.flatnonzero(slot >= 0), coupled)
    # per slot, owners sorted by step: the next owner's step is beyond the previous owner's last reader (so no two
    # overlapping intervals share a slot -- exhaustive, since the owners of a slot are totally ordered by step)
    gap = 2
    for s in range(n_slots):
        owners = coupled[slot[coupled] == s]
        owners = owners[np.argsort(step[owners], kind="stable")]
        assert len(owners) > 0
        assert (step[owners[1:]] >= last[owners[:-1]] + gap).all()
        assert len(np.unique(step[owners])) == len(owners)  # (two rows of one step never share)
    assert slot.max(initial=-1) + 1 == n_slots
    # lowest free slot first on both sides: the same slots, the same count
    assert n_slots == rn_slots and np.array_equal(slot, rslot)
    # the count is the most rows ever live (a slot is taken anew only when none is free)
    if n_steps:
        live = np.zeros(n_steps + gap + 1, np.int64)
        np.add.at(live, step[coupled], 1)
        np.add.at(live, last[coupled] + gap, -1)
        assert np.cumsum(live).max() == n_slots
    return n_slots


@pytest.fixture(scope="module")
def hier3():
    return so.build_uniform_hierarchy(3, 0.0, 1.0, 4, problem="Step16")


def equal_runs(n, blocks):
    nb = max(1, min(blocks, (n + 63) // 64))
    return [n * b // nb for b in range(nb + 1)]


@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("blocks", [1, 3, 16])
@pytest.mark.parametrize("level", [1, 2, 3, 4])
def test_slot_plan_matches_restatement(hier3, level, blocks, backward):
    m = hier3.level_matrices[level]
    br = equal_runs(m.n_rows, blocks)
    for b in range(len(br) - 1):
        check_block(m, br[b], br[b + 1], backward)


def test_live_rows_are_fewer_than_touched_rows(hier3):
    """The point of recycling: one block of level 4 touches every coupled row, but far fewer are live at once."""
    m = hier3.level_matrices[4]
    for backward in (False, True):
        step, _, _, _, n_slots = capi().ssor_slot_plan(m, 0, m.n_rows, backward)
        assert 0 < n_slots < (step >= 0).sum() // 2


class _Csr:
    """A dense matrix as host CSR; stored_zeros: positions stored with the value 0."""

    def __init__(self, dense, stored_zeros=()):
        dense = np.asarray(dense, dtype=float)
        self.n_rows = dense.shape[0]
        stored = dense != 0
        for i, j in stored_zeros:
            stored[i, j] = True
        self.rowptr = np.concatenate([[0], np.cumsum(stored.sum(axis=1))]).astype(np.int64)
        self.col = np.concatenate([np.flatnonzero(stored[i]) for i in range(self.n_rows)]).astype(np.int32)
        self.val = dense[stored]


def hand_matrix():
    """12 rows: a chain 0 - 1 - ... - 7, row 8 alone, rows 9 and 10 hang on row 0, row 11 on row 10.
    Stages: 0 | 1 9 10 | 2 11 | 3 | 4 | 5 | 6 | 7 (row 8 has none)."""
    a = 4.0 * np.eye(12)
    for i, j in [(i, i + 1) for i in range(7)] + [(0, 9), (0, 10), (10, 11)]:
        a[i, j] = a[j, i] = -1.0
    return _Csr(a, stored_zeros=[(3, 11), (11, 3)])  # (stored zeros do not couple)


def test_hand_made_matrix():
    m = hand_matrix()
    # forward: step = stage.  Row 0 is read by 1, 9, 10 (step 1), row k < 7 of the chain by k + 1, row 10 by 11 (step 2).
    # Step 3 finds the slots of rows 0 and 9 free (last reader 1), step 4 those of 1, 10, 11 (last reader 2), ...
    step, last, slot, n_steps, n_slots = capi().ssor_slot_plan(m, 0, 12, False)
    assert step.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, -1, 1, 1, 2]
    assert last.tolist() == [1, 2, 3, 4, 5, 6, 7, 7, -1, 1, 2, 2]
    assert slot.tolist() == [0, 1, 4, 0, 1, 2, 0, 1, -1, 2, 3, 5]
    assert (n_steps, n_slots) == (8, 6)
    # backward: step = 7 - stage, rows of a stage descending.  Row k > 0 of the chain is read by k - 1, rows 9 and 10 by
    # row 0 (step 7), row 11 by row 10 (step 6).
    step, last, slot, n_steps, n_slots = capi().ssor_slot_plan(m, 0, 12, True)
    assert step.tolist() == [7, 6, 5, 4, 3, 2, 1, 0, -1, 6, 6, 5]
    assert last.tolist() == [7, 7, 6, 5, 4, 3, 2, 1, -1, 7, 7, 6]
    assert slot.tolist() == [1, 5, 3, 1, 0, 2, 1, 0, -1, 4, 0, 2]
    assert (n_steps, n_slots) == (8, 6)
    for backward in (False, True):
        check_block(m, 0, 12, backward)
    # a block of its own: rows [8, 12) keep only 10 - 11
    step, last, slot, n_steps, n_slots = capi().ssor_slot_plan(m, 8, 12, False)
    assert step.tolist() == [-1, -1, 0, 1] and slot.tolist() == [-1, -1, 0, 1] and (n_steps, n_slots) == (2, 2)


def test_wide_stage_is_cut_into_steps_of_32():
    """A star: row 0 coupled to rows 1 .. 70.  Stage 1 has 70 rows = steps of 32, 32, 6; nobody reads them forward, so
    step 3 takes slots of step 1 again; backward, row 0 reads them all: 71 live."""
    a = 4.0 * np.eye(71)
    a[0, 1:] = a[1:, 0] = -1.0
    m = _Csr(a)
    step, last, slot, n_steps, n_slots = capi().ssor_slot_plan(m, 0, 71, False)
    assert n_steps == 4 and step[1:].tolist() == [1] * 32 + [2] * 32 + [3] * 6
    assert n_slots == 65  # row 0 (read until step 3) + 32 + 32: step 3 reuses slots of step 1
    assert check_block(m, 0, 71, False) == 65
    assert check_block(m, 0, 71, True) == 71


def test_bad_arguments_are_refused():
    import ctypes as C
    lib = capi().load()
    rp, col, val = np.array([0, 1, 2], np.int64), np.array([0, 1], np.int32), np.ones(2)
    p64, p32, pd = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    args = (rp.ctypes.data_as(p64), col.ctypes.data_as(p32), val.ctypes.data_as(pd))
    assert lib.gmg_ssor_slot_plan(C.c_int64(2), *args, C.c_int64(0), C.c_int64(3), C.c_int(0), None, None, None, None, None) == capi().ERR_INVALID
    assert lib.gmg_ssor_slot_plan(C.c_int64(2), *args, C.c_int64(1), C.c_int64(0), C.c_int(0), None, None, None, None, None) == capi().ERR_INVALID
    assert lib.gmg_ssor_slot_plan(C.c_int64(2), args[0], args[1], None, C.c_int64(0), C.c_int64(2), C.c_int(0), None, None, None, None, None) == capi().ERR_INVALID
    ns, nl = C.c_int64(-1), C.c_int64(-1)
    assert lib.gmg_ssor_slot_plan(C.c_int64(2), *args, C.c_int64(0), C.c_int64(2), C.c_int(1), None, None, None, C.byref(ns), C.byref(nl)) == capi().OK
    assert (ns.value, nl.value) == (0, 0)  # two rows without couplings
