"""The self-contained ranges of the four-wave SSOR sweep (option sgs_sliding, DESIGN.md 4 "One range per direction"):
a whole sweep direction of a block as ONE LDS range, y slots recycled, nothing loaded or written back at its ends.

The bar is the one of test_gpu_parity.py: a smoother step is compared BIT-EXACTLY with the oracle, whatever the plan
looks like -- self-contained ranges (default), the ranged plan (sgs_sliding = 0), an LDS budget of exactly the slots
the self-contained plan needs, two slots fewer (the largest block falls back to ranges), and 300 doubles."""
import numpy as np
import pytest

from gpu_util import capi
from oracle import gmg_oracle as go
from oracle import step50_oracle as so

pytestmark = pytest.mark.gpu

LEVEL = 4
BLOCKS = (1, 3, 16)


@pytest.fixture(scope="module")
def hier3():
    return so.build_uniform_hierarchy(3, 0.0, 1.0, 4, problem="Step16")


@pytest.fixture(scope="module")
def inputs(hier3):
    n = hier3.level_matrices[LEVEL].n_rows
    rng = np.random.default_rng(7)
    return rng.standard_normal(n), rng.standard_normal(n)


@pytest.fixture(scope="module")
def oracle_steps(hier3, inputs):
    """One smoother step of the oracle per block count and start (from zero / from u0): computed once, read-only."""
    u0, rhs = inputs
    out = {}
    for blocks in BLOCKS:
        mg = go.OracleMG(hier3, smoother=go.SSOR, ssor_blocks=blocks)
        for from_zero in (True, False):
            ref = mg.smooth(LEVEL, u0, rhs, from_zero)
            ref.setflags(write=False)
            out[blocks, from_zero] = ref
    return out


def make_context(hier, blocks, options=()):
    c = capi().Context(len(hier.level_matrices))
    c.set_tuning(ssor_blocks=blocks)
    for key, value in options:
        c.set_option(key, value)
    c.load_hierarchy(hier)
    c.set_smoother(capi().SSOR, 0.5, 2)
    return c


def step(c, inputs, from_zero):
    u0, rhs = inputs
    u, r = c.vector(len(u0), u0), c.vector(len(u0), rhs)
    c.smoother_step(LEVEL, u, r, from_zero)
    return u.download()


def coupled_rows_per_block(hier, blocks):
    """Per block of the equal-runs partition, the level rows that couple inside it (ascending)."""
    m = hier.level_matrices[LEVEL]
    n = m.n_rows
    nb = max(1, min(blocks, (n + 63) // 64))
    return [n * b // nb + np.flatnonzero(capi().ssor_slot_plan(m, n * b // nb, n * (b + 1) // nb, True)[0] >= 0) for b in range(nb)]


def blocks_with_ranges(hier, blocks):
    """Blocks that have coupled rows (the others are all pre-pass: no range)."""
    return sum(len(rows) > 0 for rows in coupled_rows_per_block(hier, blocks))


def slot_need(hier, blocks):
    c = make_context(hier, blocks)
    need = c.get_ssor_plan(LEVEL)["y_slots"]
    c.close()
    return need


@pytest.mark.parametrize("case", ["default", "sliding-off", "exact-slots", "two-slots-fewer", "300-slots"])
@pytest.mark.parametrize("blocks", BLOCKS)
def test_smoother_step_bit_exact_in_every_plan(hier3, inputs, oracle_steps, blocks, case):
    nb = blocks_with_ranges(hier3, blocks)
    options = {"default": (), "sliding-off": (("sgs_sliding", 0),), "300-slots": (("sgs_y_slots", 300),)}.get(case)
    if options is None:
        need = slot_need(hier3, blocks)
        assert need >= 66  # (below 64 the budget is clamped: the two cases would not differ)
        options = (("sgs_y_slots", need if case == "exact-slots" else need - 2),)
    c = make_context(hier3, blocks, options)
    plan = c.get_ssor_plan(LEVEL)
    n_ranges = plan["forward_ranges"] + plan["backward_ranges"]
    if case in ("default", "exact-slots"):
        # two ranges per block that has any, all self-contained
        assert (plan["forward_ranges"], plan["backward_ranges"], plan["self_contained_ranges"]) == (nb, nb, 2 * nb)
        assert plan["y_slots"] == (max(plan["max_live_forward"], plan["max_live_backward"]) + 1) // 2 * 2
        # the rows the backward records store their results to (the aux words as written into the stream, block by block):
        # per block a permutation of its coupled rows
        aux, at = c.get_ssor_backward_rows(LEVEL), 0
        for rows in coupled_rows_per_block(hier3, blocks):
            assert np.array_equal(np.sort(aux[at:at + len(rows)]), rows)
            at += len(rows)
        assert at == len(aux)
    elif case == "sliding-off":
        assert plan["self_contained_ranges"] == 0 and (plan["max_live_forward"], plan["max_live_backward"]) == (0, 0)
        assert len(c.get_ssor_backward_rows(LEVEL)) == 0
    elif case == "two-slots-fewer":
        assert plan["self_contained_ranges"] < n_ranges and n_ranges > 2 * nb  # the largest block is swept in ranges
    assert plan["forward_ranges"] >= nb and plan["backward_ranges"] >= nb and plan["steps"] > 0 and plan["stream_bytes"] > 0
    for from_zero in (True, False):
        assert np.array_equal(step(c, inputs, from_zero), oracle_steps[blocks, from_zero])
    c.close()


def test_two_applications_in_a_row_are_identical(hier3, inputs, oracle_steps):
    """The second launch finds the LDS as the first one left it: harmless (the slots are cleared once per launch)."""
    c = make_context(hier3, 3)
    first = step(c, inputs, True)
    second = step(c, inputs, True)
    assert np.array_equal(first, second) and np.array_equal(first, oracle_steps[3, True])
    c.close()


def test_switching_the_option_with_a_reupload(hier3, inputs, oracle_steps):
    c = make_context(hier3, 3)
    m = hier3.level_matrices[LEVEL]
    for on in (1, 0, 1):
        c.set_option("sgs_sliding", on)
        c.set_level_matrix(LEVEL, m)
        plan = c.get_ssor_plan(LEVEL)
        assert (plan["self_contained_ranges"] > 0) == bool(on)
        for from_zero in (True, False):
            assert np.array_equal(step(c, inputs, from_zero), oracle_steps[3, from_zero])
    c.close()


@pytest.mark.parametrize("blocks", [1, 3])
def test_whole_solve_same_bits_on_and_off(hier3, blocks):
    n = hier3.system_matrix.n_rows
    results = []
    for on in (1, 0):
        c = make_context(hier3, blocks, (("sgs_sliding", on),))
        # (level 1 is the 3 x 3 x 3 lattice: one interior row, no couplings, so its sweep is all pre-pass and has no range)
        assert c.get_ssor_plan(1)["forward_ranges"] == 0
        assert all((c.get_ssor_plan(l)["self_contained_ranges"] > 0) == bool(on) for l in range(2, len(hier3.level_matrices)))
        b, x = c.vector(n, hier3.system_rhs), c.vector(n)
        out = c.cg_solve(x, b)
        stats = c.stats()
        results.append((out["iterations"], stats.coarse_iterations, x.download()))
        assert out["status"] == 0
        c.close()
    assert results[0][0] == results[1][0] and results[0][1] == results[1][1]
    assert np.array_equal(results[0][2], results[1][2])
