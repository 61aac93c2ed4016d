"""Operators that sit exactly on the integer limits of the layout planner (csrc/gmg_layout.hpp), one on either side of each
(DESIGN.md section 34): 256 dictionary values, a slice span of 65535 columns, 96 row classes of the pattern-run kernel, 128
classes of the lattice kernel, 64 slices in a wave, the 4096-entry row window with its 1024-row cap, 1024 rows and the 12 %
padding bound.  Generators (vectorised numpy, no random numbers: tests/layout_roundtrip.cc restates them entry for entry) and the
layout each operator must get, as the bits of stats().spmv0_layout.  No fixtures, no tests; needs no GPU.

The square operators are symmetric and strictly diagonally dominant (off-diagonal entries of magnitude <= 1, 26 of them a row,
against a diagonal >= 64), so that the smoothers and the coarse CG run on them as well."""
import functools
from types import SimpleNamespace

import numpy as np

# the bits of stats().spmv0_layout
SELL, VAL8, COL16, RUNS, ROWCLASS, LATTICE = 1, 2, 4, 8, 16, 32

N_SMALL = 5037                # 78 slices of 64 rows and one of 45
N_CLASSES_ROWS = 20037        # 313 slices and one of 5 rows
N_WAVE_KEEPS = 2043 * 64      # sell_grid 8 = 32 waves: the fullest wave gets 64 slices
N_WAVE_WITHDRAWN = 2044 * 64  # ... 65 slices: the pattern-run kernel is withdrawn
EMPTY_SLICES = (0, 20, 38, 39, 77)  # first, where an XCD's eighth of the 79 slices begins, two neighbours, the last full slice


def csr(n_rows, n_cols, rowptr, col, val):
    return SimpleNamespace(n_rows=int(n_rows), n_cols=int(n_cols), rowptr=np.ascontiguousarray(rowptr, dtype=np.int64),
                           col=np.ascontiguousarray(col, dtype=np.int32), val=np.ascontiguousarray(val, dtype=np.float64), nnz=int(len(col)))


def compress(n_cols, cols, vals, mask):
    """CSR of the (row, position) grid cols / vals where mask holds, positions in stored order"""
    rowptr = np.concatenate(([0], np.cumsum(mask.sum(axis=1))))
    return csr(cols.shape[0], n_cols, rowptr, cols[mask], vals[mask])


def tridiagonal(n):
    """a small level matrix for the hierarchies that need a second level: 4 on the diagonal, -1 beside it"""
    i = np.arange(n)[:, None]
    cols = i + np.arange(-1, 2)[None, :]
    vals = np.broadcast_to(np.array([-1.0, 4.0, -1.0]), (n, 3))
    return compress(n, cols, vals, (cols >= 0) & (cols < n))


def injection(n_fine, n_coarse):
    """P[i, i % n_coarse] = 1"""
    return csr(n_fine, n_coarse, np.arange(n_fine + 1), np.arange(n_fine) % n_coarse, np.ones(n_fine))


def two_level_hierarchy(A1):
    """A1 as level 1 and system matrix over a 64-row level 0 (the hierarchy of test_smoother_epilogues_on_the_pattern_run_kernel)"""
    n = A1.n_rows
    idx = np.arange(n, dtype=np.int32)
    none = np.zeros(0, dtype=np.int32)
    return SimpleNamespace(system_matrix=A1, level_matrices=[tridiagonal(64), A1], edge_matrices=[None, None], prolongations=[injection(n, 64)],
                           copy_global=[none, idx], copy_level=[none, idx])


def one_level_hierarchy(A0):
    ident = np.arange(A0.n_rows, dtype=np.int32)
    return SimpleNamespace(system_matrix=A0, level_matrices=[A0], edge_matrices=[None], prolongations=[], copy_global=[ident], copy_level=[ident])


# ------------------------------------------------------------------------------------------------ the symmetric band of 27

def symmetric_band(n, upper, diag, empty_slices=()):
    """A[i, i + d] = A[i + d, i] = upper[i, d - 1] for d = 1 .. 13, A[i, i] = diag[i]: 27 consecutive columns a row, clipped
    at the ends (`banded` of tests/test_gpu_layouts.py).  The rows of empty_slices store nothing and no row refers to them."""
    vals = np.zeros((n, 27))
    vals[:, 13] = diag
    vals[:, 14:] = upper
    for d in range(1, 14):
        vals[d:, 13 - d] = upper[:n - d, d - 1]
    cols = np.arange(n)[:, None] + np.arange(-13, 14)[None, :]
    mask = (cols >= 0) & (cols < n)
    if len(empty_slices):
        empty = np.isin(np.arange(n) // 64, empty_slices)
        mask &= ~empty[:, None] & ~empty[np.clip(cols, 0, n - 1)]
    return compress(n, cols, vals, mask)


def dictionary_values(n_nonzero):
    """n_nonzero distinct nonzero bit patterns of magnitude <= 1 besides the diagonal 64.0 (counted): (cycle, special);
    -0.0 and the smallest subnormal are the first two of the cycle, `special` is placed by hand"""
    pool = [-0.0, 5e-324] + [s * k / 128.0 for k in range(1, 128) for s in (1.0, -1.0)]
    cycle = np.array(pool[:n_nonzero - 2])
    assert len(cycle) == n_nonzero - 2 and len({v.tobytes() for v in cycle}) == len(cycle)
    return cycle, 255.0 / 256.0


DICTIONARY_SPECIAL_ROWS = (40 * 64 + 10, 5000)  # `special` at A[r, r + 1] and A[r + 1, r]: a middle slice and the last, partial one


def dictionary_operator(n_nonzero, n=N_SMALL):
    """Case 1.  Every value of the cycle occurs within the first slices, so `special`, which first occurs in slice 40, gets
    the last code: 255 when n_nonzero = 255 (with +0.0, the padding value, 256 dictionary entries)."""
    cycle, special = dictionary_values(n_nonzero)
    k = 13 * np.arange(n)[:, None] + np.arange(13)[None, :]
    upper = cycle[k % len(cycle)]
    for r in DICTIONARY_SPECIAL_ROWS:
        upper[r, 0] = special
    return symmetric_band(n, upper, np.full(n, 64.0))


def class_vectors(K):
    """g[c, d - 1] = A[i, i + d] of a row of class c = i % K, and the K diagonals"""
    c = np.arange(K)[:, None]
    d = np.arange(1, 14)[None, :]
    small = np.array([s * k / 64.0 for k in range(1, 9) for s in (1.0, -1.0)])
    g = small[(c * (2 * d + 1) + (c // 16) * d) % 16]
    g[:, 12] = -(np.arange(K) + 1) / 256.0  # the outermost entries: K distinct values
    return g, 64.0 + np.arange(K) % 3


def class_row(K, c):
    """the 27 coefficients of a full row of class c"""
    g, diag = class_vectors(K)
    return np.concatenate(([g[(c - d) % K, d - 1] for d in range(13, 0, -1)], [diag[c]], g[c]))


def class_operator(K, n, empty_slices=()):
    """Cases 3, 4 and 5: full rows take coefficient vector row % K"""
    g, diag = class_vectors(K)
    return symmetric_band(n, g[np.arange(n) % K], diag[np.arange(n) % K], empty_slices)


# ------------------------------------------------------------------------------------------------ 11 streamed columns a row

FIVE = np.array([-1.0 / 6, -1.0 / 12, 8.0 / 3, 0.5, 1.25])


def spread_offsets(dmax):
    """offsets [lane][k] of the 11 entries of row 64 s + lane: ascending; 77 distinct ones in a slice (no column pattern);
    lane 0 holds offset 0 and lane 63 holds dmax"""
    lane = np.arange(64)[:, None]
    k = np.arange(11)[None, :]
    off = k * 6000 + 3 * (lane % 7)
    off[:, 0] = (lane[:, 0] % 7) + 1
    off[:, 10] = dmax - 1 - lane[:, 0] % 7
    off[0, 0] = 0
    off[63, 10] = dmax
    return off


def spread_values(n, few):
    k = 11 * np.arange(n)[:, None] + np.arange(11)[None, :]
    return FIVE[(k * 7 + k // 5) % 5] if few else 1.0 + k / 65536.0


def spread_operator(dmax, few, n=N_SMALL, empty_slices=()):
    """Case 2: rectangular, n_cols = n + dmax, entries at row + offset; a full slice spans 63 + dmax columns"""
    cols = np.arange(n)[:, None] + spread_offsets(dmax)[np.arange(n) % 64]
    mask = np.ones((n, 11), dtype=bool)
    if len(empty_slices):
        mask &= ~np.isin(np.arange(n) // 64, empty_slices)[:, None]
    return compress(n + dmax, cols, spread_values(n, few), mask)


DMAX_COL16 = 65472  # slice span 65535
DMAX_COL32 = 65473  # slice span 65536


# ------------------------------------------------------------------------------------------------ the padding bound, 1024 rows

def padding_operator(slices, wide_rows=0):
    """Case 7: 25 entries a row at row + 3 k, padded to 28: 28 / 25 = 1.12 exactly.  wide_rows: that many rows of slice 1
    (two are one quad) hold 29 entries: one quad more of padding for eight entries"""
    n = 64 * slices
    width = np.full(n, 25)
    width[64:64 + wide_rows] = 29
    k = np.arange(29)[None, :]
    cols = np.arange(n)[:, None] + 3 * k
    idx = 29 * np.arange(n)[:, None] + k
    return compress(n + 3 * 29, cols, FIVE[(idx * 3 + idx // 5) % 5], k < width[:, None])


def few_valued_band(n):
    """a band of 27 with five values (not symmetric): 1024 rows take the SELL layout, 1023 stay CSR"""
    cols = np.arange(n)[:, None] + np.arange(-13, 14)[None, :]
    idx = 27 * np.arange(n)[:, None] + np.arange(27)[None, :]
    vals = FIVE[(idx * 3 + idx // 5) % 5].copy()
    vals[:, 13] = 64.0
    return compress(n, cols, vals, (cols >= 0) & (cols < n))


# ------------------------------------------------------------------------------------------------ the row window

WINDOW_COLS = 6000
WINDOW_LENGTHS = (4092, 4093, 4094, 4095, 4096, 4097)


def window_rows(first_len, last_len, last_align):
    """Case 6: the row lengths of one operator.  The first row has first_len entries (it starts at entry 0); the middle holds a
    row of every length 4092 .. 4097 at every start = 0 .. 3 (mod 4), once followed by a row of 5 entries and once by three
    short rows that could share its tile, and runs of 1023, 1024 and 1025 empty rows; the last row has last_len entries and
    starts at last_align (mod 4)."""
    lens = [first_len, 2]
    nnz = first_len + 2

    def align(a):
        nonlocal nnz
        pad = (a - nnz) % 4
        if pad:
            lens.append(pad)
            nnz += pad

    for follow in ((5,), (1, 0, 2)):
        for L in WINDOW_LENGTHS:
            for a in range(4):
                align(a)
                lens.extend((L,) + follow)
                nnz += L + sum(follow)
    for run in (1023, 1024, 1025):
        lens.extend([0] * run + [3])
        nnz += 3
    align(last_align)
    lens.append(last_len)
    return np.array(lens, dtype=np.int64)


def window_operator(first_len, last_len, last_align):
    """entry j of row r sits at column (17 r) % 1200 + j + j // 7: ascending within the row, below WINDOW_COLS; the values
    alternate in sign with magnitudes in [0.5, 1.5)"""
    lens = window_rows(first_len, last_len, last_align)
    rowptr = np.concatenate(([0], np.cumsum(lens)))
    row = np.repeat(np.arange(len(lens)), lens)
    j = np.arange(rowptr[-1]) - rowptr[row]
    col = (17 * row) % 1200 + j + j // 7  # < 1200 + 4097 + 586
    assert col.max() < WINDOW_COLS
    k = np.arange(rowptr[-1])
    val = np.where(k % 2 == 0, 1.0, -1.0) * (0.5 + (k % 8191) / 8192.0)
    return csr(len(lens), WINDOW_COLS, rowptr, col, val)


def fits_window(rowptr, r):
    """a row fits the LDS window when it ends within 4096 entries of its start rounded down to 4"""
    return rowptr[r + 1] - (rowptr[r] & ~3) <= 4096


def window_tiles(rowptr):
    """The tile boundaries the planner must give, restated with the limits as plain numbers: consecutive rows while they end
    within 4096 entries of the first row's start rounded down to 4, at most 1024 rows; a row that does not fit stands alone."""
    n = len(rowptr) - 1
    tiles = [0]
    r = 0
    while r < n:
        ka = int(rowptr[r]) & ~3
        e = r + 1
        while e < n and rowptr[e + 1] - ka <= 4096 and e - r < 1024:
            e += 1
        if rowptr[e] - ka > 4096:
            e = r + 1
        tiles.append(e)
        r = e
    return tiles


def transpose(m):
    """rows and columns exchanged, the entries of a row in ascending source row"""
    row = np.repeat(np.arange(m.n_rows), np.diff(m.rowptr))
    order = np.argsort(m.col, kind="stable")
    rowptr = np.concatenate(([0], np.cumsum(np.bincount(m.col, minlength=m.n_cols))))
    return csr(m.n_cols, m.n_rows, rowptr, row[order], m.val[order])


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests

@functools.lru_cache(maxsize=None)
def operator(op):
    """the operator of a case, built once: op = (generator, argument, ...)"""
    return op[0](*op[1:])


def case(op, options=(), layout=0, pattern_slices=0, sellp_classes=None, lattice_classes=None, lattice_refused=None, square=False):
    return SimpleNamespace(op=op, options=tuple(options), layout=layout, pattern_slices=pattern_slices, sellp_classes=sellp_classes,
                           lattice_classes=lattice_classes, lattice_refused=lattice_refused, square=square)


# the operators of the cases: (generator, argument, ...)
VALUES_255, VALUES_256 = (dictionary_operator, 255), (dictionary_operator, 256)
SPAN = {(span, few): (spread_operator, dmax, few) for span, dmax in ((65535, DMAX_COL16), (65536, DMAX_COL32)) for few in (True, False)}
CLASSES = {K: (class_operator, K, N_CLASSES_ROWS) for K in (96, 97, 128, 129)}
WAVE_KEEPS, WAVE_WITHDRAWN = (class_operator, 7, N_WAVE_KEEPS), (class_operator, 7, N_WAVE_WITHDRAWN)
EMPTY_PATTERN = (class_operator, 7, N_SMALL, EMPTY_SLICES)
EMPTY_CODES, EMPTY_DOUBLES = (spread_operator, DMAX_COL16, True, N_SMALL, EMPTY_SLICES), (spread_operator, DMAX_COL32, False, N_SMALL, EMPTY_SLICES)


S8 = SELL + VAL8 + COL16
G8 = (("sell_grid", 8),)
NO_LAT = (("disable_lattice", 1),)
NO_RC = (("disable_rowclass", 1),)
NO_RUNS = (("disable_sellp", 1),)

# name -> case.  op: what makes the operator (see operator()); options: gmg_set_option pairs; layout: stats().spmv0_layout;
# pattern_slices: the slices with a column pattern ("pattern_slices a/b" of the "[gmg] operator" line; 0: every column comes from
# the stream); sellp_classes: the "row classes of the run-pattern slices" line; lattice_classes: the "lattice interior: ... classes" line; lattice_refused: the class count of the "lattice
# interior not used" line (negative: the count at which the planner gave up).
CASES = {
    # 1. value dictionary: 255 nonzero values + the padding zero = 256 codes | 257
    "values-255": case(VALUES_255, (), S8 + RUNS, 77, lattice_refused=-129, square=True),
    "values-255-per-entry-kernel": case(VALUES_255, NO_RUNS, S8, 77, lattice_refused=-129, square=True),
    "values-255-grid8": case(VALUES_255, NO_RUNS + G8, S8, 77, lattice_refused=-129, square=True),
    "values-256": case(VALUES_256, (), SELL + COL16, 77, square=True),
    "values-256-grid8": case(VALUES_256, G8, SELL + COL16, 77, square=True),
    # 2. slice span 65535 | 65536, with value codes and with doubles
    "span-65535-codes": case(SPAN[65535, True], (), S8),
    "span-65535-doubles": case(SPAN[65535, False], (), SELL + COL16),
    "span-65536-codes": case(SPAN[65536, True], (), SELL + VAL8),
    "span-65536-doubles": case(SPAN[65536, False], (), SELL),
    "span-65535-codes-grid8": case(SPAN[65535, True], G8, S8),
    "span-65535-doubles-grid8": case(SPAN[65535, False], G8, SELL + COL16),
    "span-65536-codes-grid8": case(SPAN[65536, True], G8, SELL + VAL8),
    "span-65536-doubles-grid8": case(SPAN[65536, False], G8, SELL),
    # 3. row classes: 96 | 97 for the pattern-run kernel, 128 | 129 for the lattice kernel
    "classes-96": case(CLASSES[96], (), S8 + RUNS + ROWCLASS + LATTICE, 311, 96, 96, square=True),
    "classes-96-no-lattice": case(CLASSES[96], NO_LAT, S8 + RUNS + ROWCLASS, 311, 96, square=True),
    "classes-97": case(CLASSES[97], (), S8 + RUNS + LATTICE, 311, None, 97, square=True),
    "classes-97-no-lattice": case(CLASSES[97], NO_LAT, S8 + RUNS, 311, square=True),
    "classes-128": case(CLASSES[128], (), S8 + RUNS + LATTICE, 311, None, 128, square=True),
    "classes-129": case(CLASSES[129], (), S8 + RUNS, 311, lattice_refused=-129, square=True),
    # 4. slices per wave: 32 waves, 64 | 65 slices in the fullest
    "wave-64-slices": case(WAVE_KEEPS, G8 + NO_LAT, S8 + RUNS + ROWCLASS, 2041, 7, square=True),
    "wave-64-slices-codes": case(WAVE_KEEPS, G8 + NO_LAT + NO_RC, S8 + RUNS, 2041, square=True),
    "wave-65-slices": case(WAVE_WITHDRAWN, G8 + NO_LAT, S8, 2042, square=True),
    # 5. slices without quads
    "empty-slices-lattice": case(EMPTY_PATTERN, (), S8 + RUNS + ROWCLASS + LATTICE, 73, 85, 86, square=True),
    "empty-slices-rowclass": case(EMPTY_PATTERN, NO_LAT, S8 + RUNS + ROWCLASS, 73, 85, square=True),
    "empty-slices-codes": case(EMPTY_PATTERN, NO_LAT + NO_RC, S8 + RUNS, 73, square=True),
    "empty-slices-per-entry-kernel": case(EMPTY_PATTERN, NO_LAT + NO_RUNS, S8, 73, square=True),
    "empty-slices-rowclass-grid8": case(EMPTY_PATTERN, NO_LAT + G8, S8 + RUNS + ROWCLASS, 73, 85, square=True),
    "empty-slices-rowclass-grid8-cost1": case(EMPTY_PATTERN, NO_LAT + G8 + (("sellp_cost", 1),), S8 + RUNS + ROWCLASS, 73, 85, square=True),
    "empty-slices-codes-grid8-cost16": case(EMPTY_PATTERN, NO_LAT + NO_RC + G8 + (("sellp_cost", 16),), S8 + RUNS, 73, square=True),
    "empty-slices-per-entry-kernel-grid8": case(EMPTY_PATTERN, NO_LAT + NO_RUNS + G8, S8, 73, square=True),
    "empty-slices-streamed-codes": case(EMPTY_CODES, (), S8),
    "empty-slices-streamed-doubles": case(EMPTY_DOUBLES, (), SELL),
    "empty-slices-streamed-codes-grid8": case(EMPTY_CODES, G8, S8),
    "empty-slices-streamed-doubles-grid8": case(EMPTY_DOUBLES, G8, SELL),
    # 7. entry conditions: 1024 | 1023 rows; padded entries = floor(1.12 nnz) | one quad more
    "rows-1024": case((few_valued_band, 1024), NO_LAT, S8 + RUNS + ROWCLASS, 14, 25),
    "rows-1023": case((few_valued_band, 1023), NO_LAT, 0),
    "padding-at-the-bound": case((padding_operator, 20), (), S8, 20),
    "padding-one-quad-beyond": case((padding_operator, 20, 2), (), 0),
}
