"""Small level matrices for the SSOR plan builders (option ssor_plan_device, csrc/gmg_sgs_plan.hpp), each with the outcome
that is expected of the device builder written next to it: DEVICE, or the fixed text gmg_get_ssor_plan_origin gives as the
reason why the host built the plan.  All matrices are diagonally dominant.  Needs no GPU."""
import functools
from types import SimpleNamespace

import numpy as np

DEVICE = "device"
BLOCKS = (1, 3, 20)
MAX_BLOCKS = (0, 1, 3)   # option assemble_max_blocks: by size; one workgroup; three (every grid-stride loop iterates)


def csr(n, rows):
    """rows: per row a list of (column, value) in the order they are to be stored"""
    rp = np.zeros(n + 1, dtype=np.int64)
    col, val = [], []
    for i, r in enumerate(rows):
        col += [c for c, _ in r]
        val += [v for _, v in r]
        rp[i + 1] = len(col)
    return SimpleNamespace(n_rows=n, n_cols=n, nnz=len(col), rowptr=rp, col=np.asarray(col, dtype=np.int32), val=np.asarray(val, dtype=np.float64))


def diagonal(n):
    return csr(n, [[(i, 2.0 + i % 3)] for i in range(n)])


def tridiagonal(n):
    return csr(n, [[(j, 4.0 + 0.01 * i if j == i else -1.0 - 0.001 * ((i + j) % 7)) for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)])


def pairs(n_pairs):
    rows = []
    for p in range(n_pairs):
        rows += [[(2 * p, 3.0), (2 * p + 1, -1.0 - 0.01 * p)], [(2 * p, -0.5), (2 * p + 1, 2.5)]]
    return csr(2 * n_pairs, rows)


def lattice27(k):
    idx = lambda x, y, z: (z * k + y) * k + x
    rows = []
    for z in range(k):
        for y in range(k):
            for x in range(k):
                r = []
                for dz in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            if 0 <= x + dx < k and 0 <= y + dy < k and 0 <= z + dz < k:
                                r.append((idx(x + dx, y + dy, z + dz), 30.0 if dx == dy == dz == 0 else -1.0 + 0.01 * (dx + 3 * dy + 9 * dz)))
                rows.append(r)
    return csr(k ** 3, rows)


def random_symmetric(n=3000, most=12, seed=11):
    """symmetric pattern, at most `most` off-diagonals per row, a fifth of the off-diagonal entries stored as 0.0"""
    rng = np.random.default_rng(seed)
    nb = [set() for _ in range(n)]
    for i in range(n):
        for j in rng.integers(0, n, 5):
            j = int(j)
            if j != i and len(nb[i]) < most and len(nb[j]) < most:
                nb[i].add(j)
                nb[j].add(i)
    rows = []
    for i in range(n):
        r = [(j, 0.0 if rng.random() < 0.2 else float(rng.uniform(-1, 1))) for j in sorted(nb[i])]
        rows.append(sorted(r + [(i, 20.0)]))
    return csr(n, rows)


def nonsymmetric(n=150):
    """a_ij stored, a_ji absent: a_{i, i-1} in every row, a_{i, i+5} in every third"""
    rows = []
    for i in range(n):
        r = [(i, 5.0)]
        if i > 0:
            r.append((i - 1, -1.0))
        if i % 3 == 0 and i + 5 < n:
            r.append((i + 5, -0.75))
        rows.append(sorted(r))
    return csr(n, rows)


def wide_lower(n=120, at=60, k=40):
    """row `at` with k lower neighbours: more than the 36 entries any shape of the four-wave records holds"""
    rows = [[(i, 100.0)] for i in range(n)]
    rows[at] = [(j, -1.0) for j in range(at - k, at)] + [(at, 100.0)]
    return csr(n, rows)


def too_wide(n=120, at=100, k=80):
    """row `at` with k stored entries: more than 2 * 36"""
    rows = [[(j, 4.0 if j == i else -1.0) for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)]
    rows[at] = [(j, 200.0 if j == at else -1.0) for j in range(at - k + 1, at + 1)]
    return csr(n, rows)


def unsorted(n=90, at=40):
    m = tridiagonal(n)
    k0, k1 = int(m.rowptr[at]), int(m.rowptr[at + 1])
    m.col[k0:k1] = m.col[k0:k1][::-1].copy()
    m.val[k0:k1] = m.val[k0:k1][::-1].copy()
    return m


def given_bounds(n):
    """a caller-given partition with an empty block and a one-row block"""
    return (0, 70, 70, 71, n // 2 + 5, n)


@functools.lru_cache(maxsize=None)
def adaptive_levels(name):
    """the host's level matrices (levels >= 1) of A3 / B3 of tests/mg_cases.py: hanging-node and boundary rows, stored zeros"""
    from test_level_matrix_cpu import case
    return [x.host_A for x in case(name).levels][1:]


def _case(name, make, expect=DEVICE, options=(), bounds=False, blocks=BLOCKS):
    return SimpleNamespace(name=name, make=functools.lru_cache(maxsize=None)(make), expect=expect, options=tuple(options), bounds=bounds, blocks=blocks)


# ---- planned on the device (at most 13 entries per direction: the shape g = 0, l1 = 16 always exists; every block has fewer
# rows than the y slots: nothing here can fall back)
DEVICE_CASES = [_case("diagonal-100", lambda: diagonal(100))]
DEVICE_CASES += [_case(f"tridiagonal-{n}", functools.partial(tridiagonal, n)) for n in (1, 2, 3, 4, 5, 9, 200, 5000)]
DEVICE_CASES += [
    _case("pairs-100", lambda: pairs(100)),
    _case("lattice27-9", lambda: lattice27(9)),
    _case("random-3000", random_symmetric),
    _case("nonsymmetric-150", nonsymmetric),
    _case("lattice27-9-given-rows", lambda: lattice27(9), bounds=True, blocks=(5,)),
]
DEVICE_CASES += [_case(f"{name}-level{l + 1}", functools.partial(lambda name, l: adaptive_levels(name)[l], name, l)) for name in ("A3", "B3") for l in range(2)]

# ---- planned by the host although the option is set, with the reason
FALLBACK_CASES = [
    _case("40-lower-neighbours", wide_lower, "no shape", blocks=(1,)),
    _case("80-stored-entries", too_wide, "row too wide", blocks=(1,)),
    _case("descending-columns", unsorted, "unsorted columns", blocks=(1,)),
    _case("lattice27-9-64-slots", lambda: lattice27(9), "block does not fit", (("sgs_y_slots", 64),), blocks=(1, 3)),
    _case("balanced", lambda: lattice27(9), "balanced partition", (("ssor_balanced", 1),), blocks=(3,)),
    _case("sliding-off", lambda: lattice27(9), "option sgs_sliding unset", (("sgs_sliding", 0),), blocks=(1,)),
    _case("dep", lambda: lattice27(9), "option sgs_dep set", (("sgs_dep", 1),), blocks=(1,)),
]


def runs(cases):
    """(case, blocks) for every block count the rows allow (the library clamps B to (n + 63) / 64)"""
    out = []
    for c in cases:
        for b in c.blocks:
            if c.bounds or b == 1 or c.name.startswith(("A3", "B3")) or b <= (c.make().n_rows + 63) // 64:
                out.append((c, b))
    return out


def run_id(run):
    return f"{run[0].name}-B{run[1]}"
