"""The device-resident coarse CG (run_cg_chunks, the fused and the three-kernel iteration with its ring of directions, the
odd-length tails, cg_open_iteration) and the entry conditions of gmg_cg_solve against tests/cg_reference.py.

Every solve is compared with the reference in return code, iteration count, residual (1e-9 relative) and x (64 S max|x|, S
the spread of the reference's three tiers, computed by cg_reference alone); the stopping iteration of a case is set through
the tolerance (cg_reference.target_tol), so that solves end on, before and after the ring boundaries at 8, 16 and 24 and on,
before and after the end of an enqueued chunk.  tests/test_cg_reference_cpu.py proves every case targetable in every tier
and sensitive: the smallest step alpha_j d_j of any case is more than 100 tolerances."""
import numpy as np
import pytest

import cg_reference as R
from gpu_util import capi

pytestmark = pytest.mark.gpu

# path -> (operator, cg_variant asked for, variant that must run, predicate on spmv0_layout)
PATHS = {
    "fused-csr": ("csr", 1, 1, lambda lay: lay == 0),
    "fused-sell": ("sell", 1, 1, lambda lay: lay == 5),
    "three-csr": ("csr", 2, 2, lambda lay: lay == 0),
    "three-sell": ("sell", 2, 2, lambda lay: lay == 5),
    "three-lattice": ("lattice", 2, 2, lambda lay: lay >= 1 and bool((lay - 1) & 32) and lay != 127),
    "formed": ("formed", 0, 2, lambda lay: lay == 127),
    "fused-band9": ("band9", 1, 1, lambda lay: lay == 0),
    "three-band9": ("band9", 2, 2, lambda lay: lay == 0),
}
PATH_KS = {"three-lattice": R.LATTICE_KS, "formed": R.FORMED_KS, "fused-band9": (8, 9), "three-band9": (8, 9)}

_worst = {"ratio": 0.0, "case": None}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print(f"\nworst |x - x_ref| / tolerance over this file: {_worst['ratio']:.3g} at {_worst['case']}")


def make_context(name, variant_asked, layout_ok=None, comm=False):
    m, _ = R.operator(name)
    c = capi().Context(1)
    if comm:
        c.comm_init(0, 1, capi().Context.unique_id())
        c.set_global_sizes(m.n_rows, m.n_rows)
    c.set_tuning(cg_variant=variant_asked)
    if name == "formed":
        c.set_level_matrix_lattice(0, R.FORMED_SHAPE, R.formed_cell_matrix())
    else:
        c.set_level_matrix(0, m)
    if layout_ok is not None:
        lay = int(c.stats().spmv0_layout)
        assert layout_ok(lay), f"{name}: level 0 is stored in layout {lay}, not the one this case is written for"
    return c


def solve(c, b, tol, max_it, chunk, variant_asked):
    c.set_tuning(coarse_chunk=chunk, cg_variant=variant_asked)
    c.set_coarse(tol, max_it)
    vb, vx = c.vector(len(b), b), c.vector(len(b), np.full(len(b), np.nan))
    it, res, rc = c.coarse_solve(vx, vb)
    x = vx.download()
    vb.free(); vx.free()
    return x, it, res, rc


def check(got, ref, name, what, variant=None, c=None):
    x, it, res, rc = got
    want_rc = capi().OK if ref.status == R.OK else capi().ERR_COARSE_NOCONV
    assert rc == want_rc, (what, rc, it, res)
    assert it == ref.iterations, (what, it, ref.iterations)
    assert abs(res - ref.res) <= 1e-9 * ref.res, (what, res, ref.res)
    scale = np.abs(ref.x).max()
    tol = R.x_tolerance(name) * scale
    err = np.abs(x - ref.x).max() if not np.isnan(x).any() else np.inf
    if tol > 0 and err / tol > _worst["ratio"]:
        _worst["ratio"], _worst["case"] = float(err / tol), what
    assert err <= tol, (what, f"|x - x_ref| = {err:.3e} = {err / tol:.3g} tolerances, first at {int(np.argmax(~(np.abs(x - ref.x) <= tol)))}")
    if variant is not None:
        assert int(c.stats().coarse_variant) == variant, what


def same_bits(a, b, what):
    assert a[1:] == b[1:] and np.array_equal(a[0], b[0]), (what, a[1:], b[1:], int(np.sum(a[0] != b[0])))


_fresh = {}


def fresh(path, kind, k):
    """the case on a context of its own, default chunk: (x, iterations, res, rc)"""
    key = (path, kind, k)
    if key not in _fresh:
        name, asked, variant, layout_ok = PATHS[path]
        c = make_context(name, asked, layout_ok)
        if kind == "stop":
            tol, max_it, b = R.stop_case(name, k)[0], 1000, R.rhs(name)
        elif kind == "refuse":
            tol, max_it, b = R.REFUSE_TOL, k, R.rhs(name)
        else:
            tol, max_it, b = 1e-10, 1000, np.zeros(R.operator(name)[0].n_rows)
        _fresh[key] = solve(c, b, tol, max_it, 0, asked)
        c.close()
    return _fresh[key]


@pytest.mark.parametrize("path", list(PATHS))
def test_stopping_iteration_by_chunk_and_path(path):
    """k on, before and after the ring boundaries x chunk 0 (predicted from the previous solve), 1, 3, 8 and k itself (the
    chunk ends with the converging iteration; its convergence is seen by the first kernel of the next chunk): the reference's
    result every time, and the same bits whatever the chunk and whatever ran on the context before."""
    name, asked, variant, layout_ok = PATHS[path]
    c = make_context(name, asked, layout_ok)
    b = R.rhs(name)
    ks = PATH_KS.get(path, R.STOP_KS)
    for k in ks:
        tol, ref = R.stop_case(name, k)
        first = None
        for chunk in dict.fromkeys((0, 1, 3, 8, k)):
            got = solve(c, b, tol, 1000, chunk, asked)
            check(got, ref, name, (path, k, chunk), variant, c)
            if first is None:
                first = got
            same_bits(got, first, (path, k, chunk))
        if k in (ks[0], 9, 11, ks[-1]):
            same_bits(fresh(path, "stop", k), first, (path, k, "fresh context"))
    c.close()


@pytest.mark.parametrize("path", ["fused-csr", "three-csr"])
def test_solve_sequence_on_one_context(path):
    """25, 3, 20, zero rhs, 9, refused at 5, 17 on one context with the predicted first chunk: too long and too short a
    prediction, and whatever ring and state keep from the solve before.  Every result is the one a fresh context gives, bit
    for bit; the counters add up."""
    name, asked, variant, layout_ok = PATHS[path]
    c = make_context(name, asked, layout_ok)
    c.stats_reset()
    total = 0
    for kind, k in R.SEQUENCE:
        if kind == "stop":
            tol, ref = R.stop_case(name, k)
            got = solve(c, R.rhs(name), tol, 1000, 0, asked)
        elif kind == "refuse":
            tol, ref = R.refused_case(name, k)
            got = solve(c, R.rhs(name), tol, k, 0, asked)
        else:
            got = solve(c, np.zeros(len(R.rhs(name))), 1e-10, 1000, 0, asked)
            assert got[1:] == (0, 0.0, capi().OK) and not got[0].any()
            ref = None
        if ref is not None:
            check(got, ref, name, (path, "sequence", kind, k), variant, c)
        same_bits(got, fresh(path, kind, k), (path, "sequence", kind, k))
        total += got[1]
    st = c.stats()
    assert int(st.coarse_solves) == len(R.SEQUENCE) and int(st.coarse_iterations) == total == 25 + 3 + 20 + 0 + 9 + 5 + 17
    assert int(st.coarse_enqueued) >= int(st.coarse_iterations)
    c.close()


@pytest.mark.parametrize("path", ["fused-csr", "three-csr", "fused-sell", "three-sell"])
def test_refused_solves_leave_the_iterate(path):
    """max_it reached: GMG_ERR_COARSE_NOCONV, iterations == max_it, and dst holds the iterate after max_it steps (deal.II
    leaves it in dst when SolverControl throws), with the chunk below, equal to and above max_it.  The context solves on."""
    name, asked, variant, layout_ok = PATHS[path]
    c = make_context(name, asked, layout_ok)
    b = R.rhs(name)
    for max_it in R.REFUSE_MAX_ITS:
        tol, ref = R.refused_case(name, max_it)
        assert ref.status == R.NOCONV and ref.iterations == max_it
        first = None
        for chunk in dict.fromkeys((0, max(1, max_it // 2), max_it, max_it + 3)):
            got = solve(c, b, tol, max_it, chunk, asked)
            check(got, ref, name, (path, "max_it", max_it, chunk), variant, c)
            first = first or got
            same_bits(got, first, (path, "max_it", max_it, chunk))
    tol, ref = R.stop_case(name, 8)
    check(solve(c, b, tol, 1000, 0, asked), ref, name, (path, "after refused solves"), variant, c)
    c.close()


@pytest.mark.parametrize("path", ["fused-csr", "three-csr"])
def test_nothing_to_do(path):
    name, asked, variant, layout_ok = PATHS[path]
    m, _ = R.operator(name)
    c = make_context(name, asked, layout_ok)
    for chunk in (0, 1):
        x, it, res, rc = solve(c, np.zeros(m.n_rows), 1e-10, 1000, chunk, asked)
        assert (it, res, rc) == (0, 0.0, capi().OK) and not x.any() and not np.signbit(x).any()
        b = R.rhs(name)
        ref = R.cg(m, b, 1e3, 1000, tier="ld")  # |b| from the long-double tier: the closest to the exact norm
        assert ref.iterations == 0 and ref.status == R.OK
        x, it, res, rc = solve(c, b, 1e3, 1000, chunk, asked)
        assert (it, rc) == (0, capi().OK) and not x.any()
        assert abs(res - ref.res) <= 1e-15 * ref.res, (res, ref.res)
        assert int(c.stats().coarse_variant) == variant
    c.close()


@pytest.mark.parametrize("path", ["fused-csr", "three-csr"])
def test_nan_in_the_rhs_is_refused_at_once(path):
    """res is NaN at the first opening: SolverControl fails with 0 iterations (an ordinary, bounded error path)"""
    name, asked, variant, layout_ok = PATHS[path]
    m, _ = R.operator(name)
    b = R.rhs(name).copy()
    b[m.n_rows // 3] = np.nan
    ref = R.cg(m, b, 1e-10, 1000)
    assert (ref.iterations, ref.status) == (0, R.NOCONV)
    c = make_context(name, asked, layout_ok)
    x, it, res, rc = solve(c, b, 1e-10, 1000, 0, asked)
    assert (it, rc) == (0, capi().ERR_COARSE_NOCONV) and np.isnan(res) and not x.any()
    tol, ref = R.stop_case(name, 7)
    check(solve(c, R.rhs(name), tol, 1000, 0, asked), ref, name, (path, "after a NaN rhs"), variant, c)
    c.close()


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("n", R.LENGTHS)
def test_lengths_around_the_pair_and_workgroup_boundaries(n, variant):
    """the update kernels work on pairs with a grid sized by n / 2; the odd last element belongs to thread 0 of workgroup 0"""
    name = f"tri{n}"
    m, _ = R.operator(name)
    k = R.length_k(n)
    tol, ref = R.stop_case(name, k)
    c = make_context(name, variant, lambda lay: lay == 0)
    first = None
    for chunk in (0, 1, k):
        got = solve(c, R.rhs(name), tol, 1000, chunk, variant)
        check(got, ref, name, (name, variant, chunk), variant, c)
        first = first or got
        same_bits(got, first, (name, variant, chunk))
    if n == 1:
        assert first[1] == 1 and abs(first[0][0] - R.rhs(name)[0] / m.val[0]) <= 4 * 2.0 ** -53 * abs(first[0][0])
    c.close()


@pytest.mark.parametrize("n,variant", [(R.VARIANT_SIZES[0], 1), (R.VARIANT_SIZES[1], 2)])
def test_variant_chosen_by_size(n, variant):
    name = f"tri{n}"
    tol, ref = R.stop_case(name, R.VARIANT_K)
    c = make_context(name, 0, lambda lay: lay == 0)
    check(solve(c, R.rhs(name), tol, 1000, 0, 0), ref, name, (name, "cg_variant 0"), variant, c)
    c.close()


def test_one_rank_communicator():
    """a partitioned level 0 over RCCL: the all-reduced scalars replace the partials and no chunk is enqueued speculatively"""
    name = "csr"
    c = make_context(name, 0, lambda lay: lay == 0, comm=True)
    assert c.comm_info()["level0_partitioned"]
    ref_ctx = {}
    for k in R.COMM_KS:
        tol, ref = R.stop_case(name, k)
        for chunk in (0, 3):
            got = solve(c, R.rhs(name), tol, 1000, chunk, 0)
            check(got, ref, name, ("one rank", k, chunk), 2, c)
            same_bits(got, ref_ctx.setdefault(k, got), ("one rank", k, chunk))
    c.close()


# ---------------------------------------------------------------------------------------------- the outer CG

PRECOND = {"identity": "PRECOND_IDENTITY", "jacobi": "PRECOND_JACOBI"}


@pytest.fixture(scope="module")
def outer():
    m, _ = R.operator("csr")
    c = capi().Context(1)
    c.set_system_matrix(m)
    yield c, m, R.rhs("csr"), float(R.cg(m, R.rhs("csr"), np.inf, 0, tier="ld").res)
    c.close()


def outer_solve(c, b, x0, tol, norm_b, max_it, pc):
    vb, vx = c.vector(len(b), b), c.vector(len(b), x0)
    r = c.cg_solve(vx, vb, rel_tol=tol / norm_b if norm_b else tol, max_it=max_it, precond=getattr(capi(), PRECOND[pc]))
    r["x"] = vx.download()
    vb.free(); vx.free()
    return r


def outer_check(r, ref, what):
    want = capi().OK if ref.status == R.OK else capi().ERR_OUTER_NOCONV
    assert r["status"] == want and r["iterations"] == ref.iterations, (what, r["status"], r["iterations"], ref.iterations)
    assert abs(r["starting_value"] - ref.history[0]) <= 1e-9 * ref.history[0], what
    assert abs(r["convergence_value"] - ref.res) <= 1e-9 * ref.res, what
    tol = R.x_tolerance("csr") * np.abs(ref.x).max()
    err = np.abs(r["x"] - ref.x).max()
    if err / tol > _worst["ratio"]:
        _worst["ratio"], _worst["case"] = float(err / tol), what
    assert err <= tol, (what, f"{err / tol:.3g} tolerances")


@pytest.mark.parametrize("pc", list(PRECOND))
def test_outer_cg_entry_conditions(outer, pc):
    c, m, b, norm_b = outer
    n = m.n_rows
    # zero start and a random start vector, stopping at iteration OUTER_K
    for start in ("zero", "random"):
        tol, ref = R.stop_case("csr", R.OUTER_K, pc, start)
        x0 = R.x_start("csr") if start == "random" else np.zeros(n)
        outer_check(outer_solve(c, b, x0, tol, norm_b, 500, pc), ref, ("outer", pc, start))
    # a start vector that already meets the tolerance: nothing is done to it
    x0, tol, ref = R.converged_start_case(pc)
    r = outer_solve(c, b, x0, tol, norm_b, 500, pc)
    assert (r["status"], r["iterations"]) == (capi().OK, 0) and np.array_equal(r["x"], x0)
    # (|A x0 - b| is what cancellation leaves of terms of the size of |b|: compared on that scale)
    assert abs(r["starting_value"] - ref.res) <= 1e-12 * norm_b and r["convergence_value"] == r["starting_value"]
    # b = 0, x0 = 0
    r = outer_solve(c, np.zeros(n), np.zeros(n), 1e-8, 0.0, 500, pc)
    assert (r["status"], r["iterations"], r["starting_value"], r["convergence_value"]) == (capi().OK, 0, 0.0, 0.0) and not r["x"].any()
    # max_it reached: the iterate stays in x
    tol, ref = R.refused_case("csr", R.OUTER_MAX_IT, pc)
    outer_check(outer_solve(c, b, np.zeros(n), tol, norm_b, R.OUTER_MAX_IT, pc), ref, ("outer", pc, "max_it"))
