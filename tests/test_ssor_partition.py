"""Where the SSOR blocks are cut (gmg_ssor_balance_rows, DESIGN.md 4 "Block boundaries"): the balanced cuts of the
library, checked on the host -- the routine needs neither a context nor a device.  The reference's ranks sweep the
rows they own (src/step-50.cc:722-723, :970-973), p4est's cell-balanced chunks (:120-122); equal runs of rows put most of
the Gauss-Seidel chain of an adaptive level into the first blocks."""
import numpy as np
import pytest

from gpu_util import capi, pkg
from oracle import gmg_oracle as go
from oracle import step50_oracle as so

STEP_NS, BYTES_PER_NS, ROW_BYTES, ENTRY_BYTES, ROWS_PER_STEP = 240.0, 48.0, 64, 28, 32


def block_model(m, rb, re, use_values=True):
    """(sub-steps, stream bytes, cost in us) of rows [rb, re), restated: stage(i) = 1 + max stage(j) over the j in [rb, i)
    coupled to i through a nonzero a_ij or a_ji; both directions take every stage in steps of <= 32 rows; coupled rows
    stream 64 bytes plus 28 per in-block entry; uncoupled rows cost nothing."""
    rp, col, val = np.asarray(m.rowptr, np.int64), np.asarray(m.col, np.int64), np.asarray(m.val)
    r = np.repeat(np.arange(rb, re), np.diff(rp[rb:re + 1]))
    c, v = col[rp[rb]:rp[re]], val[rp[rb]:rp[re]]
    keep = (c >= rb) & (c < re) & ((v != 0) if use_values else True)
    r, c = r[keep], c[keep]
    ent = np.bincount(r - rb, minlength=re - rb)
    off = r != c
    lo, hi = np.minimum(r[off], c[off]), np.maximum(r[off], c[off])
    coupled = np.zeros(re - rb, bool)
    coupled[lo - rb] = True
    coupled[hi - rb] = True
    order = np.argsort(hi, kind="stable")
    lo, hi = lo[order], hi[order]
    starts = np.searchsorted(hi, np.arange(rb, re + 1))
    stage = np.zeros(re - rb, np.int64)
    for i in range(re - rb):
        if starts[i + 1] > starts[i]:
            stage[i] = stage[lo[starts[i]:starts[i + 1]] - rb].max() + 1
    cnt = np.bincount(stage[coupled]) if coupled.any() else np.zeros(0, np.int64)
    steps = 2 * int(np.sum((cnt + ROWS_PER_STEP - 1) // ROWS_PER_STEP))
    nbytes = int(np.sum(ROW_BYTES + ENTRY_BYTES * ent[coupled]))
    return steps, nbytes, (STEP_NS * steps + nbytes / BYTES_PER_NS) * 1e-3


def ratio(c):
    c = np.asarray(c, dtype=float)
    return c.max() / c.mean()


@pytest.fixture(scope="module")
def hier3():
    return so.build_uniform_hierarchy(3, 0.0, 1.0, 4, problem="Step16")


def config3_cycle4_hierarchy():
    """BASELINE config 3 (1000 atoms) at adaptive cycle 4, built on the host as test_cluster_cycles.py builds its
    hierarchies; the earlier cycles are solved by the oracle.  Level 1 has 44 084 rows."""
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=5.0, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous",
                             cycles=5, r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0,
                             smoother="SSOR", refinement_estimator="Kelly"))
    p.set_nacl_atoms(5)
    for cycle in range(5):
        p.run_cycle(cycle, on_device=False)
        h = p.hierarchy()
        if cycle < 4:
            p.finish_cycle_with(go.OracleMG(h, smoother=go.SSOR).solve(h.system_rhs, x0=p.vector("initial_guess"))["x"])
    assert [m.n_rows for m in h.level_matrices] == [226981, 44084, 14336]
    return h


@pytest.fixture(scope="module")
def adaptive_level():
    return config3_cycle4_hierarchy().level_matrices[1]


@pytest.mark.parametrize("level", [2, 3, 4])
@pytest.mark.parametrize("blocks", [1, 2, 3, 7, 64])
def test_boundaries_well_formed(hier3, level, blocks):
    m = hier3.level_matrices[level]
    n = m.n_rows
    br, cost = capi().ssor_balance_rows(m, blocks)
    assert len(br) == blocks + 1 and len(cost) == blocks
    assert br[0] == 0 and br[-1] == n and np.all(np.diff(br) >= 0)
    used = min(blocks, (n + 63) // 64)  # the clamp of the equal runs: no more than one block per 64 rows
    assert np.all(br[used:] == n) and np.all(cost[used:] == 0)
    assert np.count_nonzero(np.diff(br)) <= used
    again = capi().ssor_balance_rows(m, blocks)
    assert np.array_equal(br, again[0]) and np.array_equal(cost, again[1])


@pytest.mark.parametrize("use_values", [True, False])
@pytest.mark.parametrize("level,blocks", [(3, 1), (3, 4), (4, 1), (4, 5), (4, 16)])
def test_costs_match_restated_recurrence(hier3, level, blocks, use_values):
    m = hier3.level_matrices[level]
    br, cost = capi().ssor_balance_rows(m, blocks, use_values=use_values)
    want = [block_model(m, br[b], br[b + 1], use_values)[2] for b in range(blocks)]
    np.testing.assert_allclose(cost, want, rtol=1e-12, atol=0)


def test_invalid_input_rejected():
    lib = capi().load()
    import ctypes as C

    rp = np.array([0, 1, 2], dtype=np.int64)
    col = np.array([0, 5], dtype=np.int32)  # column out of range
    br = np.zeros(3, dtype=np.int64)
    p64, p32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    rc = lib.gmg_ssor_balance_rows(C.c_int64(2), rp.ctypes.data_as(p64), col.ctypes.data_as(p32), None, C.c_int(2), br.ctypes.data_as(p64), None)
    assert rc == capi().ERR_INVALID
    col[1] = 1
    rc = lib.gmg_ssor_balance_rows(C.c_int64(2), rp.ctypes.data_as(p64), col.ctypes.data_as(p32), None, C.c_int(0), br.ctypes.data_as(p64), None)
    assert rc == capi().ERR_INVALID


def test_balanced_beats_equal_rows_on_adaptive_level(adaptive_level):
    m = adaptive_level
    n = m.n_rows
    for B in (2, 8, 20):
        br, cost = capi().ssor_balance_rows(m, B)
        assert br[-1] == n and np.count_nonzero(np.diff(br)) == B
        assert ratio(cost) <= 1.15, (B, cost)
        np.testing.assert_allclose(cost, [block_model(m, br[b], br[b + 1])[2] for b in range(B)], rtol=1e-12, atol=0)
        eq = [n * b // B for b in range(B + 1)]
        eq_cost = [block_model(m, eq[b], eq[b + 1])[2] for b in range(B)]
        # the chain sits in the low row numbers: equal runs are 3.0x (B = 8) / 3.8x (B = 20) off their mean here (B = 2: 1.6x,
        # out of at most 2)
        assert ratio(eq_cost) >= (1.5 if B == 2 else 1.8), (B, eq_cost)
        assert max(cost) < max(eq_cost) / (1.4 if B == 2 else 2.5)


def test_prm_key_values():
    """"SSOR block partition" takes "equal rows" (the default) or "balanced"; anything else is rejected."""
    S = pkg().step50
    S.Problem(S.prm_text(problem="Step16", dim=2, ssor_partition="balanced"))
    S.Problem(S.prm_text(problem="Step16", dim=2, ssor_partition="equal rows"))
    with pytest.raises(RuntimeError, match="SSOR block partition"):
        S.Problem(S.prm_text(problem="Step16", dim=2, ssor_partition="rows"))
