"""Matrices and the plain-Python restatement for the rows of the SSOR sweep scheduled by slack (gmg_ssor_pack_levels, option
sgs_pack; DESIGN.md 4 "Rows scheduled by slack"), shared by tests/test_ssor_pack_cpu.py and tests/test_gpu_ssor_pack.py.
Needs no GPU.

The restatement, from the definition:
  height(i) = 0 if row i has no higher coupled neighbour, else 1 + max height(k) over its higher neighbours;
  step t = 0, 1, ...: a row is ready when all its lower coupled neighbours lie in steps < t; the step takes at most 32 ready
  rows, height descending, then row ascending;  level(i) = the row's step."""
from types import SimpleNamespace

import numpy as np

import ssor_plan_cases as spc
import ssor_shape_cases as K

ROWS_PER_STEP = 32


def comb():
    """60 rows: rows 0 .. 19 are a chain, rows 20 .. 59 are each coupled to row 0 only.  (Row 0 has 42 entries in the backward
    direction, more than a record of the four-wave sweep holds: the library sweeps this matrix with the one-wave plan, which
    keeps the stages.  The levels are defined and checked all the same; comb_two_hubs is the comb the four-wave plan takes.)"""
    nb = [set() for _ in range(60)]
    for i in range(19):
        nb[i].add(i + 1)
    for i in range(20, 60):
        nb[0].add(i)
    return K.from_pattern(nb, 1)


def comb_two_hubs():
    """55 rows: rows 0 .. 19 are a chain, row 20 is a second row without lower neighbours, rows 21 .. 37 hang on row 0 and rows
    38 .. 54 on row 20.  Stage 1 has 35 rows (row 1 and the 34 teeth): 21 steps by stages, 20 packed -- and every row fits a
    record of the four-wave sweep (the widest has 19 entries in a direction, at most 18 of them updated one step earlier)."""
    nb = [set() for _ in range(55)]
    for i in range(19):
        nb[i].add(i + 1)
    for t in range(17):
        nb[0].add(21 + t)
        nb[20].add(38 + t)
    return K.from_pattern(nb, 4)


def star():
    """row 0 coupled to rows 1 .. 70 (the star of tests/test_ssor_slots_cpu.py): nothing can move"""
    return K.from_pattern([set(range(1, 71))] + [set() for _ in range(70)], 2)


def delayed_leaves(depth=20):
    """32 chains side by side, `depth` rows long; every chain row has a leaf that reads it.  The chain rows fill every packed
    step, so the leaves wait until the chains have ended and the rows they read stay live: the packed levels need far more
    y slots than the stages, which take a depth's leaves right after its chain rows.  Rows by depth: 32 chain rows, 32 leaves."""
    nb = [set() for _ in range(64 * depth)]
    for d in range(depth):
        for k in range(32):
            if d:
                nb[64 * d + k].add(64 * (d - 1) + k)
            nb[64 * d + 32 + k].add(64 * d + k)
    return K.from_pattern(nb, 3)


def wide_late_span(n=128):
    """Packed levels with a step no shape holds, although the stages have a four-wave plan.  Row 40 is coupled to rows 0 .. 29,
    rows 30 .. 39 each to row 50 + k; every other row is uncoupled.  Stage 0 has 40 rows: by stages rows 0 .. 31 are step 0,
    rows 32 .. 39 step 1 and row 40 (stage 1) comes in step 2, none of its columns updated one step earlier.  Packed, rows
    0 .. 31 (height 1) are level 0 and row 40 is ready for level 1: all 30 columns are late, first to last more than the 28
    T1 slots of any shape.  The block must then be planned from its stages."""
    nb = [set() for _ in range(n)]
    nb[40] |= set(range(30))
    for k in range(10):
        nb[30 + k].add(50 + k)
    return K.from_pattern(nb, 5)


MATRICES = {
    "comb": comb,
    "comb-two-hubs": comb_two_hubs,
    "star": star,
    "delayed-leaves": delayed_leaves,
    "wide-late-span": wide_late_span,
    "tridiagonal-200": lambda: spc.tridiagonal(200),
    "lattice27-9": lambda: spc.lattice27(9),
    "lattice27-17": lambda: spc.lattice27(17),
    "random-3000": spc.random_symmetric,
    "A3-level1": lambda: spc.adaptive_levels("A3")[0],
    "A3-level2": lambda: spc.adaptive_levels("A3")[1],
    "B3-level1": lambda: spc.adaptive_levels("B3")[0],
    "B3-level2": lambda: spc.adaptive_levels("B3")[1],
}
ONE_BLOCK_ONLY = ("comb", "comb-two-hubs", "star", "wide-late-span")   # too few rows, or a case made for one block


def equal_runs(n, blocks):
    nb = max(1, min(blocks, (n + 63) // 64))
    return [n * b // nb for b in range(nb + 1)]


def diag_block(m, rb, re):
    """rows and columns [rb, re) of m as a matrix of its own"""
    rp, col, val = np.asarray(m.rowptr, np.int64), np.asarray(m.col, np.int64), np.asarray(m.val)
    rows = np.repeat(np.arange(rb, re), np.diff(rp[rb:re + 1]))
    c, v = col[rp[rb]:rp[re]], val[rp[rb]:rp[re]]
    keep = (c >= rb) & (c < re)
    rp_b = np.zeros(re - rb + 1, np.int64)
    np.cumsum(np.bincount(rows[keep] - rb, minlength=re - rb), out=rp_b[1:])
    return SimpleNamespace(n_rows=re - rb, n_cols=re - rb, nnz=int(keep.sum()), rowptr=rp_b, col=(c[keep] - rb).astype(np.int32), val=v[keep])


def neighbours(m, rb, re):
    """(lower, higher) coupled neighbours per row of the block [rb, re), local numbers: stored value != 0, column in the block,
    through a_ij or a_ji"""
    nb = re - rb
    lower, higher = [set() for _ in range(nb)], [set() for _ in range(nb)]
    rp = m.rowptr
    for i in range(rb, re):
        for k in range(int(rp[i]), int(rp[i + 1])):
            c = int(m.col[k])
            if rb <= c < re and c != i and m.val[k] != 0:
                lo, hi = min(i, c) - rb, max(i, c) - rb
                lower[hi].add(lo)
                higher[lo].add(hi)
    return lower, higher


def restated(m, rb, re):
    """(level per row, -1 without couplings; levels; stage per row; stage-by-stage steps of a direction) of the block"""
    lower, higher = neighbours(m, rb, re)
    nb = re - rb
    coupled = [bool(lower[i] or higher[i]) for i in range(nb)]
    stage = [-1] * nb
    for i in range(nb):
        if coupled[i]:
            stage[i] = 1 + max((stage[j] for j in lower[i]), default=-1)
    height = [0] * nb
    for i in range(nb - 1, -1, -1):
        height[i] = 1 + max((height[k] for k in higher[i]), default=-1)
    level = [-1] * nb
    waiting = [len(lower[i]) for i in range(nb)]
    ready = [i for i in range(nb) if coupled[i] and not lower[i]]
    t = 0
    while ready:
        ready.sort(key=lambda i: (-height[i], i))
        taken, ready = ready[:ROWS_PER_STEP], ready[ROWS_PER_STEP:]
        for i in taken:
            level[i] = t
        for i in taken:
            for k in higher[i]:
                waiting[k] -= 1
                if waiting[k] == 0:
                    ready.append(k)
        t += 1
    counts = np.bincount(np.asarray([s for s in stage if s >= 0], dtype=np.int64)) if any(coupled) else np.zeros(0, np.int64)
    stage_steps = int(((counts + ROWS_PER_STEP - 1) // ROWS_PER_STEP).sum())
    return np.asarray(level), t, np.asarray(stage), stage_steps
