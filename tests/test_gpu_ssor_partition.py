"""SSOR blocks on caller-given and balanced row partitions, on the MI355X.  The oracle cuts only equal runs of rows, so
the reference for other boundaries is composed from it block by block: the reference's rank-local smoother
(src/step-50.cc:970-973) on a block is the oracle's SSOR on that diagonal block with the other blocks' columns dropped,
and the residual steps of MGSmootherPrecondition run on the whole level matrix (oracle/gmg_oracle.c: smooth)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import rel_close
from gpu_util import capi, pkg
from oracle import gmg_oracle as go
from oracle import step50_oracle as so
from test_gpu_two_ranks import run_ranks
from test_ssor_partition import config3_cycle4_hierarchy, ratio

pytestmark = pytest.mark.gpu

OMEGA, STEPS = 0.5, 2


def _diag_block(m, rb, re):
    rp, col, val = np.asarray(m.rowptr, np.int64), np.asarray(m.col, np.int64), np.asarray(m.val)
    rows = np.repeat(np.arange(rb, re), np.diff(rp[rb:re + 1]))
    c, v = col[rp[rb]:rp[re]], val[rp[rb]:rp[re]]
    keep = (c >= rb) & (c < re)
    rp_b = np.zeros(re - rb + 1, np.int64)
    np.cumsum(np.bincount(rows[keep] - rb, minlength=re - rb), out=rp_b[1:])
    return SimpleNamespace(n_rows=re - rb, n_cols=re - rb, nnz=int(keep.sum()), rowptr=rp_b, col=(c[keep] - rb).astype(np.int32), val=v[keep])


class ComposedOracle:
    """smooth() of the oracle with SSOR blocks at arbitrary boundaries (empty blocks allowed)."""

    def __init__(self, A, bounds):
        self.A, self.bounds = A, [int(b) for b in bounds]
        self.blocks = []
        for rb, re in zip(self.bounds[:-1], self.bounds[1:]):
            if re == rb:
                continue
            Ab = _diag_block(A, rb, re)
            h = SimpleNamespace(system_matrix=Ab, level_matrices=[Ab], edge_matrices=[None], prolongations=[],
                                copy_global=[np.zeros(0, np.int32)], copy_level=[np.zeros(0, np.int32)])
            self.blocks.append((rb, re, go.OracleMG(h, smoother=go.SSOR, omega=OMEGA, steps=1)))

    def apply_inverse(self, r):
        y = np.zeros(self.A.n_rows)
        for rb, re, mg in self.blocks:
            y[rb:re] = mg.smooth(0, np.zeros(re - rb), r[rb:re], True)
        return y

    def smooth(self, u, rhs, from_zero):
        u = np.array(u, dtype=np.float64)
        first = 0
        if from_zero:
            u = self.apply_inverse(rhs)
            first = 1
        for _ in range(first, STEPS):
            res = rhs - go.spmv(self.A, u)
            u = u + self.apply_inverse(res)
        return u


@pytest.fixture(scope="module")
def hier3():
    return so.build_uniform_hierarchy(3, 0.0, 1.0, 4, problem="Step16")


@pytest.fixture(scope="module")
def hier_adaptive():
    return config3_cycle4_hierarchy()


def _context(hier, variant="default", blocks=None, level_rows=None, balanced=False):
    c = capi().Context(len(hier.level_matrices))
    if blocks:
        c.set_tuning(ssor_blocks=blocks)
    if balanced:
        c.set_ssor_partition(capi().SSOR_PARTITION_BALANCED)
    if variant == "ranges":
        c.set_option("sgs_y_slots", 300)
    elif variant == "one-wave":
        c.set_option("sgs_disable_phase", 1)
    for level, rows in (level_rows or {}).items():
        c.set_ssor_block_rows(level, rows)
    c.load_hierarchy(hier)
    c.set_smoother(capi().SSOR, OMEGA, STEPS)
    return c


def _smooth(c, level, u0, rhs, from_zero):
    u, r = c.vector(len(u0), u0), c.vector(len(rhs), rhs)
    c.smoother_step(level, u, r, from_zero)
    out = u.download()
    u.free()
    r.free()
    return out


def test_composed_oracle_is_the_oracle_on_equal_runs(hier3):
    level, B = 4, 3
    A = hier3.level_matrices[level]
    n = A.n_rows
    rng = np.random.default_rng(3)
    u0, rhs = rng.standard_normal(n), rng.standard_normal(n)
    comp = ComposedOracle(A, [n * b // B for b in range(B + 1)])
    mg = go.OracleMG(hier3, smoother=go.SSOR, ssor_blocks=B)
    for from_zero in (True, False):
        assert np.array_equal(comp.smooth(u0, rhs, from_zero), mg.smooth(level, u0, rhs, from_zero))


@pytest.mark.parametrize("variant", ["default", "ranges", "one-wave"])
@pytest.mark.parametrize("which", ["hier3", "adaptive"])
def test_explicit_boundaries_bit_exact(request, which, variant):
    """Irregular cuts: a one-row block, an empty block, cuts that are not multiples of 64."""
    hier = request.getfixturevalue("hier3" if which == "hier3" else "hier_adaptive")
    level = 4 if which == "hier3" else 1
    A = hier.level_matrices[level]
    n = A.n_rows
    bounds = [0, 1, 1, 700, 2333, 4000, n] if which == "hier3" else [0, 1, 1, 5002, 17777, 30011, n]
    c = _context(hier, variant, level_rows={level: bounds})
    br, steps = c.get_ssor_partition(level)
    assert list(br) == bounds and len(steps) == len(bounds) - 1 and steps[0] == 0 and steps[1] == 0
    comp = ComposedOracle(A, bounds)
    rng = np.random.default_rng(11)
    u0, rhs = rng.standard_normal(n), rng.standard_normal(n)
    for from_zero in (True, False):
        assert np.array_equal(_smooth(c, level, u0, rhs, from_zero), comp.smooth(u0, rhs, from_zero)), from_zero
    c.close()


def test_explicit_equal_runs_match_ssor_blocks(hier3):
    level, B = 4, 5
    n = hier3.level_matrices[level].n_rows
    rng = np.random.default_rng(5)
    u0, rhs = rng.standard_normal(n), rng.standard_normal(n)
    a = _context(hier3, blocks=B)
    b = _context(hier3, level_rows={level: [n * k // B for k in range(B + 1)]})
    assert np.array_equal(a.get_ssor_partition(level)[0], b.get_ssor_partition(level)[0])
    assert np.array_equal(a.get_ssor_partition(level)[1], b.get_ssor_partition(level)[1])
    for from_zero in (True, False):
        assert np.array_equal(_smooth(a, level, u0, rhs, from_zero), _smooth(b, level, u0, rhs, from_zero))
    a.close()
    b.close()


def test_balanced_partition_on_adaptive_level(hier_adaptive):
    level, B = 1, 8
    A = hier_adaptive.level_matrices[level]
    n = A.n_rows
    eq = _context(hier_adaptive, blocks=B)
    c = _context(hier_adaptive, blocks=B, balanced=True)
    br_eq, steps_eq = eq.get_ssor_partition(level)
    br, steps = c.get_ssor_partition(level)
    assert list(br_eq) == [n * k // B for k in range(B + 1)]
    assert np.array_equal(br, capi().ssor_balance_rows(A, B)[0])  # the host routine is what the plan used
    print(f"sub-steps per block, equal rows {list(steps_eq)} (longest / mean {ratio(steps_eq):.2f}), "
          f"balanced {list(steps)} ({ratio(steps):.2f})")
    assert ratio(steps) <= 1.25
    assert ratio(steps_eq) >= 1.8
    comp = ComposedOracle(A, br)
    rng = np.random.default_rng(13)
    u0, rhs = rng.standard_normal(n), rng.standard_normal(n)
    for from_zero in (True, False):
        assert np.array_equal(_smooth(c, level, u0, rhs, from_zero), comp.smooth(u0, rhs, from_zero))
    eq.close()
    c.close()


def test_invalid_boundaries_rejected(hier3):
    c = capi().Context(len(hier3.level_matrices))
    n = hier3.level_matrices[4].n_rows
    lib = c.L
    for level, rows in ((4, [0, 100, 50, n]), (4, [1, 100, n]), (0, [0, hier3.level_matrices[0].n_rows])):
        with pytest.raises(capi().GMGError) as e:
            c.set_ssor_block_rows(level, rows)
        assert e.value.code == capi().ERR_INVALID
    c.set_ssor_block_rows(4, [0, 100, n - 1])  # wrong last entry: found when the matrix arrives
    with pytest.raises(capi().GMGError) as e:
        c.load_hierarchy(hier3)
    assert e.value.code == capi().ERR_INVALID
    nb = ctypes.c_int(0)
    assert lib.gmg_get_ssor_partition(c.h, 4, ctypes.byref(nb), None, None) == capi().ERR_INVALID  # no plan was built
    with pytest.raises(capi().GMGError):
        c.set_ssor_partition(2)
    c.set_ssor_block_rows(4, [])  # cleared: the equal runs again
    c.load_hierarchy(hier3)
    assert list(c.get_ssor_partition(4)[0]) == [0, n]
    c.close()


def _cycles(partition):
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=5.0, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous",
                             cycles=5, r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0,
                             smoother="SSOR", refinement_estimator="Kelly", ssor_blocks=4, ssor_partition=partition))
    p.set_nacl_atoms(5)
    return [p.run_cycle(c, on_device=True) for c in range(5)]


def test_adaptive_solve_converges_balanced():
    """atoms1000, SSOR in 4 blocks through the prm path: balanced cuts keep the outer counts within one of the equal runs
    (the reference moves 6 -> 7 on p4est's partition, tests/gaussian-charges.mpirun=3.output:92)."""
    rows, bal = _cycles("equal rows"), _cycles("balanced")
    print("outer iterations, equal rows", [r["cg_iterations"] for r in rows], "balanced", [r["cg_iterations"] for r in bal])
    for a, b in zip(rows, bal):
        assert a["dofs_by_level"] == b["dofs_by_level"]
        assert abs(a["cg_iterations"] - b["cg_iterations"]) <= 1
        assert rel_close(a["sol_l2"], b["sol_l2"], 6)


def test_two_ranks_balanced(golden_dir, tmp_path, monkeypatch):
    """Two ranks sharing the GPU, one balanced block each: what one process computes with the same two blocks."""
    env = {"GMG_OPTIONS": "ssor_balanced=1"}
    ranks = run_ranks(2, golden_dir, tmp_path, monkeypatch, env_extra=env, blocks=2)
    one = run_ranks(0, golden_dir, tmp_path, monkeypatch, env_extra=env, blocks=2)[0]
    for reps in ranks:
        for r, g in zip(reps, one):
            assert r["dofs_by_level"] == g["dofs_by_level"] and r["cg_iterations"] == g["cg_iterations"]
            for k in ("sol_l1", "sol_l2", "sol_linf", "starting_value", "refine_threshold", "energy_total"):
                assert rel_close(r[k], g[k], 9), (k, r[k], g[k])
