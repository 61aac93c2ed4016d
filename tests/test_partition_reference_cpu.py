"""tests/partition_reference.py against the host code production uses (Problem.localize, gmg_partition_range), and the proof
that the partitioned SpMV cases of tests/test_gpu_ranks_reference.py notice a wrong ghost tail: with the ranks emulated in numpy
(owned slice, ghost tail filled from ghost_global) every mutation of the tail moves some row of the product by 100 times the
bound that row is checked with on the GPU, or more.  The ratios are printed ("[ranks]", run with -s)."""
import ctypes as C

import numpy as np
import pytest

import partition_reference as PR
import rank_cases as RC
from gpu_util import capi, pkg

SENSITIVITY = 100.0
FIELDS = ("n_rows", "n_cols", "nnz", "row_begin")
ARRAYS = ("rowptr", "col", "val", "neighbor_rank", "send_count", "send_idx", "recv_count", "ghost_global")


@pytest.fixture(scope="module")
def step16():
    """the Step16 3D problem of tests/test_distributed_cpu.py: its system matrix and its level 0"""
    S = pkg().step50
    pkg().build.build_all()
    p = S.Problem(S.prm_text(left=0, right=1, problem="Step16", dim=3, bc="Homogeneous", cycles=1, global_refinement=3))
    p.run_cycle(0, on_device=False)
    yield p
    p.close()


@pytest.mark.parametrize("n_ranks", [1, 2, 3, 5])
@pytest.mark.parametrize("kind", ["system", "level"])
def test_localize_equals_the_host_code(step16, kind, n_ranks):
    G = step16.matrix("system") if kind == "system" else step16.matrix("level", 0)
    for rank in range(n_ranks):
        host = step16.localize(kind, 0, rank, n_ranks)
        mine = PR.localize(G, rank, n_ranks)
        for f in FIELDS:
            assert int(getattr(host, f)) == int(getattr(mine, f)), (kind, n_ranks, rank, f)
        for a in ARRAYS:
            assert np.array_equal(np.asarray(getattr(host, a)), np.asarray(getattr(mine, a))), (kind, n_ranks, rank, a)
        assert (PR.owned_range(G.n_rows, rank, n_ranks)[0], mine.n_rows) == (host.row_begin, host.n_rows)


def test_owned_range_equals_gmg_partition_range():
    """a host call of the library: no GPU is touched"""
    lib = capi().load()
    for n_ranks in range(1, 9):
        for n in (0, 1, n_ranks - 1, n_ranks, n_ranks + 1, 4097):
            covered = 0
            for rank in range(n_ranks):
                b, e = C.c_int64(-1), C.c_int64(-1)
                assert lib.gmg_partition_range(C.c_int64(n), C.c_int(rank), C.c_int(n_ranks), C.byref(b), C.byref(e)) == 0
                assert (b.value, e.value) == PR.owned_range(n, rank, n_ranks), (n, rank, n_ranks)
                assert b.value == covered and e.value - b.value <= PR.chunk(n, n_ranks)
                covered = e.value
            assert covered == n


def locs_of(name, n_ranks):
    return [PR.localize(RC.operator(name), r, n_ranks) for r in range(n_ranks)]


def test_plans_are_consistent_and_have_the_advertised_shape():
    for name, n_ranks in RC.spmv_cases():
        locs = locs_of(name, n_ranks)
        assert all(l.n_rows >= 1 for l in locs)
        for r, l in enumerate(locs):
            assert list(l.neighbor_rank) == sorted(set(int(s) for s in l.neighbor_rank)) and r not in l.neighbor_rank
            so = 0
            for s, sc in zip(l.neighbor_rank, l.send_count):
                peer = locs[int(s)]
                k = list(peer.neighbor_rank).index(r)   # listed on both sides, also where one count is zero
                lo, hi = PR.segments(peer)[k]
                assert hi - lo == sc and np.array_equal(l.row_begin + l.send_idx[so:so + sc], peer.ghost_global[lo:hi])
                so += sc
            assert so == len(l.send_idx) and l.n_cols == l.n_rows + int(l.recv_count.sum())
    # one entry per neighbour
    for n_ranks in RC.RANKS:
        for r, l in enumerate(locs_of("tri1031", n_ranks)):
            assert list(l.neighbor_rank) == [s for s in (r - 1, r + 1) if 0 <= s < n_ranks]
            assert np.all(l.send_count == 1) and np.all(l.recv_count == 1)
    # the band wider than a chunk on four ranks: a rank with three neighbours, non-adjacent ones among them, and a pair of
    # ranks that are no neighbours
    wide = locs_of("wide", 4)
    assert [list(l.neighbor_rank) for l in wide] == [[1, 2], [0, 2, 3], [0, 1, 3], [1, 2]]
    assert all(np.all(l.send_count > 0) and np.all(l.recv_count > 0) for l in wide)
    # two decoupled blocks: nobody has a neighbour
    assert all(len(l.neighbor_rank) == 0 and l.n_cols == l.n_rows == RC.BLOCK_ROWS for l in locs_of("blocks", 2))
    # the one-sided pattern: the last rank sends and receives nothing, the first receives and sends nothing
    for n_ranks in RC.RANKS:
        one = locs_of("unsym", n_ranks)
        assert list(one[-1].neighbor_rank) == [n_ranks - 2] and one[-1].recv_count[0] == 0 and one[-1].send_count[0] == 7
        assert list(one[0].neighbor_rank) == [1] and one[0].send_count[0] == 0 and one[0].recv_count[0] == 7
        assert one[-1].n_cols == one[-1].n_rows


def emulate(locs, x, tail=None):
    """the partitioned product: every rank's local operator on [owned | ghost tail]; tail(rank, loc, ghosts) may spoil the tail"""
    y = np.zeros(len(x))
    for r, l in enumerate(locs):
        ghosts = x[l.ghost_global]
        if tail is not None:
            ghosts = tail(r, l, ghosts.copy())
        xl = np.concatenate([x[l.row_begin:l.row_begin + l.n_rows], ghosts])
        y[l.row_begin:l.row_begin + l.n_rows] = PR.row_sums(l, xl)[0].astype(np.float64)
    return y


def mutations(locs, x_before):
    """name -> tail function, for the mutations this partition can show at all"""
    out = {}
    if any(len(l.ghost_global) for l in locs):
        out["tail left at zero"] = lambda r, l, g: np.zeros_like(g)
        out["tail of the previous round"] = lambda r, l, g: x_before[l.ghost_global]
        seg = {r: next((s for s in PR.segments(l) if s[1] - s[0] > 0), None) for r, l in enumerate(locs)}

        def shifted(r, l, g):
            lo, hi = seg[r] if seg[r] else (0, 0)
            g[lo:hi] = np.roll(g[lo:hi], 1) if hi - lo > 1 else g[lo:hi] + 1.0   # (one entry: it holds its neighbour's value)
            return g

        out["one segment shifted by one entry"] = shifted
    if any(np.sum(l.recv_count > 0) >= 2 for l in locs):
        def exchanged(r, l, g):
            segs = [s for s in PR.segments(l) if s[1] - s[0] > 0]
            if len(segs) < 2:
                return g
            (a0, a1), (b0, b1) = segs[0], segs[1]
            return np.concatenate([g[:a0], g[b0:b1], g[a1:b0], g[a0:a1], g[b1:]])

        out["two neighbours' segments exchanged"] = exchanged
    return out


@pytest.mark.parametrize("name,n_ranks", RC.spmv_cases() + RC.layout_spmv_cases(), ids=lambda v: str(v))
def test_every_spmv_case_notices_a_wrong_ghost_tail(name, n_ranks):
    """Per (operator, N, vector, mutation): some row of the mutated product is SENSITIVITY bounds or more away from the true
    row sum, the bound being the one the GPU test checks that row with.  The unmutated emulation is within the bound.
    "blocks" has no ghost tail: no mutation applies to it, and what it is there for -- ranks without neighbours that stay in
    step with the rounds that follow -- is seen by the products and reductions that follow it on the same context.  On two
    ranks nobody has two neighbours, so nothing can be exchanged there; the exchange is shown on three and four ranks.
    The operators of RC.LAYOUT_OPERATORS (tests/test_gpu_ranks_layouts.py) are held to the same: their GPU test asserts this
    bound next to bit equality, so every mutation fails both."""
    m = RC.operator(name)
    locs = locs_of(name, n_ranks)
    X = RC.spmv_vectors(name)
    low = {}
    for i in range(RC.N_SPMV_VECTORS):
        y, bound = PR.spmv_bound(m, X[i])
        assert np.all(bound > 0)
        assert np.all(np.abs(emulate(locs, X[i]) - y) <= bound)
        muts = mutations(locs, X[i - 1])
        assert (name == "blocks") == (len(muts) == 0)
        assert ("two neighbours' segments exchanged" in muts) == (n_ranks > 2 and name != "unsym")
        for what, tail in muts.items():
            ratio = float(np.max(np.abs(emulate(locs, X[i], tail) - y) / bound))
            low[what] = min(low.get(what, np.inf), ratio)
            assert ratio >= SENSITIVITY, (name, n_ranks, i, what, ratio)
    print(f"\n[ranks] SpMV sensitivity {name} on {n_ranks} ranks (|difference| / bound, worst row, min over the vectors): "
          + (", ".join(f"{k} {v:.1e}" for k, v in low.items()) if low else "no ghost tail, no mutation applies"))


# ------------------------------------------------------------------------------------------------ device layouts (section 33)

def test_the_layout_table_holds_every_layout():
    """RC.LAYOUTS by itself: each layout tests/test_gpu_ranks_layouts.py is about is expected of some rank, so equality with the
    table cannot be met by ranks that fell back to the CSR kernel"""
    for n in RC.RANKS:
        lat = RC.LAYOUTS["lattice", n]
        assert all(e.level0 & 32 and e.window[0] == {2: 8, 3: 5, 4: 3}[n] for e in lat)    # fewer plane steps than XCD slabs for N > 2
        assert [bool(e.level0 & 8) for e in lat] == [True] + [n == 2] * (n - 1)             # lattice plans without the pattern-run plan
        assert all(e.system == "hybrid" and e.level0 == RC.CSR for e in RC.LAYOUTS["hybspd", n])
        assert all(e.level0 == RC.FULL and e.window[0] > 100 for e in RC.LAYOUTS["bandfew", n])
        assert all(e.level0 == RC.SELL_FP64 for e in RC.LAYOUTS["banddist", n])
        for name in RC.LAYOUT_OPERATORS:     # every rank owns enough rows for a SELL plan to be tried at all, and has ghosts
            assert all(l.n_rows >= 1024 and len(l.ghost_global) > 0 for l in locs_of(name, n)), (name, n)
        # a wide row of the hybrid operator refers to every other rank
        assert all(len(l.neighbor_rank) == n - 1 for l in locs_of("hybspd", n))
    assert [e.level0 for e in RC.LAYOUTS["lat21", 4]] == [RC.CSR, RC.FULL, RC.FULL, RC.CSR]
    assert [e.system for e in RC.LAYOUTS["lat21", 4]] == ["hybrid", "sell", "sell", "hybrid"]


LATTICE_STRIDES = {"lattice": (37, 37 * 23), "lat21": (21, 21 * 17), "bandfew": (3, 9)}


def lattice_row_sets(loc, nx, nxy):
    """numpy stand-in of the lattice kernel's two row sets for a lexicographic numbering (the window spans whole planes,
    W = nxy): `fast` = the longest run [R0, R1) of rows at least reach + 2 from either end whose stored columns are all owned
    and among the 27 lattice offsets -- the rows the marching waves write --, `generic` = the rows of the 64-row slices that
    hold any other row -- what lattice_generic_slice walks, writing where its `valid` mask lets it.  Returns (K, R0, R1, fast,
    generic)."""
    n, reach = loc.n_rows, nxy + nx + 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(loc.rowptr))
    t = loc.col.astype(np.int64) - row + reach
    entry_ok = (loc.col < n) & (t >= 0) & (t // nxy <= 2) & ((t % nxy) // nx <= 2) & ((t % nxy) % nx <= 2)
    bad = np.zeros(n, dtype=np.int64)
    np.add.at(bad, row, ~entry_ok)
    r = np.arange(n)
    ok = (bad == 0) & (r >= reach + 2) & (r + reach < n)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], ok.astype(np.int8), [0]])))
    begins, ends = edges[0::2], edges[1::2]
    longest = int(np.argmax(ends - begins))     # (the first of equal ones, as the planner)
    R0, R1 = int(begins[longest]), int(ends[longest])
    fast = (r >= R0) & (r < R1)
    slice_has_other = np.zeros((n + 63) // 64, dtype=bool)
    np.logical_or.at(slice_has_other, r // 64, ~fast)
    return -(-(R1 - R0) // nxy), R0, R1, fast, slice_has_other[r // 64]


@pytest.mark.parametrize("name,n_ranks", [(name, n) for n in RC.RANKS for name in LATTICE_STRIDES if any(e.window for e in RC.LAYOUTS[name, n])],
                         ids=lambda v: str(v))
def test_a_broken_interior_mask_of_the_generic_slices_is_noticed(name, n_ranks):
    """The interior rows inside a generic slice written twice, the generic slice's value last (lattice_generic_slice without
    its `valid` mask).  The two row sets come from the numpy stand-in above, which must give the K, R0 and R1 of RC.LAYOUTS.

    In a product the second write carries the same bits as the first -- the streams of a generic slice hold its interior rows
    too, and both kernels sum a row in its stored order, which is what their bit equality with the CSR product on one rank
    says -- so y = A x cannot show this mutation and need not.  What the mask guards is the coarse CG's d.h: a row written
    twice is summed twice.  Shown on the first iteration of the coarse solves of the layout group (d = b): the mutated
    alpha = g.g / d.h moves x_1 = alpha d, the solve that stops at iteration 1, by SENSITIVITY tolerances on x or more, with
    the mask broken on any single rank.  The opposite defect, a mask that is too wide, leaves rows unwritten: y is pre-filled
    with NaN and the product test requires that none is left."""
    nx, nxy = LATTICE_STRIDES[name]
    m = RC.operator(name)
    locs = locs_of(name, n_ranks)
    coarse = name in RC.layout_coarse_operators(n_ranks)
    if coarse:
        b = RC.rhs(name)
        h = PR.row_sums(m, b)[0].astype(np.float64)
        dh, ref = float(b @ h), RC.stop_case(name, 1)[1]
        tol = RC.x_tolerance(name) * np.abs(ref.x).max()
        assert ref.iterations == 1 and np.abs(ref.x - (b @ b) / dh * b).max() <= tol
    low, n_twice = np.inf, []
    for r, l in enumerate(locs):
        want = RC.LAYOUTS[name, n_ranks][r].window
        if want is None:
            continue
        K, R0, R1, fast, generic = lattice_row_sets(l, nx, nxy)
        assert (K, R0, R1) == (want[0], want[2], want[3]), (name, n_ranks, r, (K, R0, R1), want)
        twice = np.flatnonzero(fast & generic)
        n_twice.append(len(twice))
        assert len(twice) > 0 and np.all(l.col[np.concatenate([np.arange(l.rowptr[i], l.rowptr[i + 1]) for i in np.flatnonzero(fast)])] < l.n_rows)
        if coarse:
            g = l.row_begin + twice
            x1 = (b @ b) / (dh + float(b[g] @ h[g])) * b
            low = min(low, float(np.abs(x1 - ref.x).max() / tol))
    assert n_twice, (name, n_ranks)
    if coarse:
        assert low >= SENSITIVITY, (name, n_ranks, low)
    print(f"\n[ranks] broken interior mask, {name} on {n_ranks} ranks: rows written twice per rank {n_twice}"
          + (f", |x_1 - x_ref| / tolerance at least {low:.1e}" if coarse else " (no coarse solve on this operator)"))
