"""The device layouts of row-partitioned operators on 2, 3 and 4 ranks.  The operators of
tests/test_gpu_ranks_reference.py are so small that every rank's rows stay on the CSR row-window kernel; here every rank owns
1100 to 8100 rows and the planner gives it what production gets: SELL-64 streams (fp64 values or value codes), the pattern-run
kernel with row classes, the plane-by-plane lattice kernel with the rows that touch ghost columns in its generic slices -- with
and without the pattern-run plan, with fewer plane steps than XCD slabs --, the hybrid layout, and on four ranks of the
21 x 17 x 40 lattice two CSR ranks next to two lattice ranks in one collective product.

Launcher, worker and conventions are those of tests/test_gpu_ranks_reference.py: fresh interpreters sharing the one GPU over the
peer transport, one launch per (group, N), shared by the tests that read it; a launch that hangs or loses a rank to a signal
ends the launches of both modules.  Every test first requires that every rank reported the layout tests/rank_cases.py expects
(stats().spmv0_layout, the "[gmg]   layout" word and the lattice window of the debug_upload lines): nothing here can pass on
the CSR kernel.

Products: bit for bit the oracle's CSR product of the global matrix, for every option set -- the one-rank tests hold each of
these kernels to that, localization keeps a row's stored order, and pattern slices and lattice-interior rows exist only where
all columns are owned and ascending -- with the bound gamma_(k+1) sum_j |a_ij x_j| against numpy.longdouble as the floor beside
it.  Solves: check and outer_check of tests/test_gpu_coarse_cg.py, unchanged."""
import re

import numpy as np
import pytest

import cg_reference as R
import partition_reference as PR
import rank_cases as RC
from gpu_util import capi
from oracle import gmg_oracle as go
from test_gpu_coarse_cg import outer_check, same_bits
from test_gpu_ranks_reference import check_info, coarse_check, coarse_result, joined, ranks, same_on_all, say  # noqa: F401  (ranks: the fixture)

pytestmark = pytest.mark.gpu

WINDOW = re.compile(r"lattice interior: nx \d+ nxy \d+ rows \[(\d+), (\d+)\) of \d+, \d+ classes, (\d+) columns x (\d+) steps, (\d+) segments per XCD slab")


def parse_upload(log):
    """(layout words, lattice window (K, C, R0, R1) or None, segments per XCD slab or None) of one upload's debug lines"""
    lines = str(log).splitlines()
    words = [ln.split("layout", 1)[1].split()[0].rstrip(":") for ln in lines if "[gmg]   layout" in ln]
    found = [WINDOW.search(ln) for ln in lines if "[gmg]   lattice interior:" in ln]
    assert len(found) <= 1 and all(found), lines
    if not found:
        return words, None, None
    r0, r1, c, k, s = (int(v) for v in found[0].groups())
    return words, (k, c, r0, r1), s


def require_layout(res, name, n_ranks, rank, variant, prefix, system=True, level0=True):
    """the layout this rank reported for `name` is the one of RC.LAYOUTS"""
    want = RC.expected_layout(name, n_ranks, rank, variant)
    what = (name, n_ranks, rank, variant)
    segments = dict(RC.LAYOUT_VARIANTS[name])[variant].get("lattice_segments", 0) if name in RC.LAYOUT_VARIANTS else 0
    if level0:
        assert int(res[prefix + "layout"][0]) == want.level0, (what, int(res[prefix + "layout"][0]), want.level0)
        words, window, s = parse_upload(res[prefix + "lvlog"])
        assert words == ["sell" if want.level0 else "csr"] and window == want.window, (what, words, window, want.window)
        assert bool(want.level0 & 32) == (window is not None)
    if system:
        words, window, s = parse_upload(res[prefix + "syslog"])
        assert words == [want.system] and window == want.window, (what, words, window, want.window)
        if want.system == "hybrid":
            assert "val8 1" in str(res[prefix + "syslog"]), what
    if want.window is not None and segments:     # the option reached the plan: min(asked, plane steps of an XCD slab)
        assert s == min(segments, max(1, want.window[0] // 8)), (what, s)


@pytest.mark.parametrize("n_ranks", RC.RANKS)
def test_every_rank_reports_the_expected_layout(ranks, n_ranks):
    """stats().spmv0_layout, the layout word and the lattice window of every upload of the product group: per operator, per
    option set that steers the plan, per rank.  disable_lattice takes the window away and leaves the rest; lattice_segments
    shows in the plan's segment count."""
    per_rank = ranks("layout_spmv", n_ranks)
    n_checked = 0
    for name in RC.LAYOUT_OPERATORS:
        for variant, options in RC.LAYOUT_VARIANTS[name]:
            if variant != "default" and not any(k in RC.UPLOAD_OPTIONS for k in options):
                continue
            for r, res in enumerate(per_rank):
                require_layout(res, name, n_ranks, r, variant, f"{name}_{variant}_")
                n_checked += 1
    reported = {int(res[f"{name}_default_layout"][0]) for name in RC.LAYOUT_OPERATORS for res in per_rank}
    assert {RC.CSR, RC.FULL, RC.SELL_FP64} <= reported and (n_ranks == 2 or RC.LATTICE_PLAIN in reported), reported
    if n_ranks == 4:    # the ranks of one collective product run different kernels
        assert [int(res["lat21_default_layout"][0]) for res in per_rank] == [RC.CSR, RC.FULL, RC.FULL, RC.CSR]
    print(f"\n[ranks-gpu] layouts on {n_ranks} ranks: {n_checked} uploads as expected; level-0 layouts reported {sorted(reported)}")


@pytest.mark.parametrize("name", RC.LAYOUT_OPERATORS)
@pytest.mark.parametrize("n_ranks", RC.RANKS)
def test_partitioned_product_on_its_layout(ranks, n_ranks, name):
    """gmg_spmv(GMG_SYSTEM) and gmg_spmv(0) on owned rows, five vectors in a row per option set, y pre-filled with NaN: the
    ranks' y joined has no NaN left, equals the oracle's product of the global matrix bit for bit and lies within the bound
    gamma_(k+1) sum_j |a_ij x_j| of the row's numpy.longdouble sum.  The reduction that follows each operator shows the ranks
    in step."""
    per_rank = ranks("layout_spmv", n_ranks)
    ld = np.longdouble
    m = RC.operator(name)
    X = RC.spmv_vectors(name)
    uploaded = "default"
    worst, n_products = 0.0, 0
    refs = [(go.spmv(m, X[i]),) + PR.spmv_bound(m, X[i]) for i in range(RC.N_SPMV_VECTORS)]
    for variant, options in RC.LAYOUT_VARIANTS[name]:
        if any(k in RC.UPLOAD_OPTIONS for k in options):
            uploaded = variant
        for r, res in enumerate(per_rank):
            require_layout(res, name, n_ranks, r, uploaded, f"{name}_{uploaded}_")
        for i, (ref, y, bound) in enumerate(refs):
            for which in ("sys", "lv"):
                got = joined(per_rank, f"{name}_{variant}_{which}{i}")
                what = (n_ranks, name, variant, which, i)
                assert got.shape == ref.shape and not np.isnan(got).any(), (what, int(np.isnan(got).sum()), int(np.argmax(np.isnan(got))))
                err = np.abs(got.astype(ld) - y).astype(np.float64)
                worst = max(worst, float(np.max(err / bound)))
                assert np.all(err <= bound), (what, int(np.argmax(err / bound)), float(np.max(err / bound)))
                bad = np.nonzero(got != ref)[0]
                assert bad.size == 0, (what, bad.size, bad[:10], got[bad[:3]], ref[bad[:3]])
                n_products += 1
    xs, ys = zip(*[RC.reduce_vectors(257, r) for r in range(n_ranks)])
    a, b = np.concatenate(xs).astype(ld), np.concatenate(ys).astype(ld)
    got = same_on_all(per_rank, f"{name}_dot")[0]
    assert abs(float(ld(got) - np.sum(a * b))) <= float(PR.gamma(len(a)) * np.sum(np.abs(a * b))), (n_ranks, name)
    print(f"\n[ranks-gpu] {name} on {n_ranks} ranks: {n_products} products bit-equal to the oracle's; error / bound max {worst:.3g}")


@pytest.mark.parametrize("n_ranks", RC.RANKS)
def test_coarse_cg_on_a_partitioned_lattice_plan(ranks, n_ranks):
    """gmg_coarse_solve with level 0 = the owned rows of the 37 x 23 x 19 lattice (spmv_lattice_kernel<2>: the generic slices
    serve the rows that touch ghost columns, d.h over owned rows only, one partial per workgroup into peer_allsum_kernel; the
    direction kernels of the neighbours fill the ghost tail) and, on four ranks, of the 21 x 17 x 40 lattice (two ranks on the
    CSR kernel, two on the lattice kernel, in one solve): stopping iterations on and next to the ring boundaries, chunks 0, 1
    and 3, through check of tests/test_gpu_coarse_cg.py.  Scalars equal on every rank, the same bits with every chunk."""
    per_rank = ranks("layout_coarse", n_ranks)
    worst = {}
    for name in RC.layout_coarse_operators(n_ranks):
        for r, res in enumerate(per_rank):
            require_layout(res, name, n_ranks, r, "default", f"{name}_", system=False)
        for k in RC.LAYOUT_COARSE_KS[name]:
            tol, ref = RC.stop_case(name, k)
            first = None
            for chunk in RC.COARSE_CHUNKS:
                got = coarse_result(per_rank, f"{name}_k{k}_c{chunk}")
                worst[name] = max(worst.get(name, 0.0), coarse_check(got, ref, name, (n_ranks, name, k, chunk)))
                first = first or got
                same_bits(got, first, (n_ranks, name, k, chunk))
        assert all(int(res[f"{name}_variant"][0]) == 2 for res in per_rank)
        for res in per_rank:
            check_info(res[f"{name}_info"], n_ranks, True, ring="fine-grained")
    for res in per_rank:
        check_info(res["comm_info"], n_ranks, True, ring="fine-grained")
    say(f"coarse CG on lattice plans on {n_ranks} ranks", **worst)


@pytest.mark.parametrize("pc", ["identity", "jacobi"])
@pytest.mark.parametrize("n_ranks", RC.RANKS)
def test_outer_cg_on_a_partitioned_hybrid_system(ranks, n_ranks, pc):
    """gmg_cg_solve on owned rows of the hybrid operator (spmv_hybrid_kernel reading a ghost tail that refers to every other
    rank) through outer_check of tests/test_gpu_coarse_cg.py: zero and random start, b = 0, max_it reached"""
    per_rank = ranks("layout_outer", n_ranks)
    C = capi()
    name = RC.LAYOUT_OUTER
    for r, res in enumerate(per_rank):
        require_layout(res, name, n_ranks, r, "default", "", level0=False)

    def result(what):
        status, it, r0, r = same_on_all(per_rank, f"{pc}_{what}_m")
        return {"status": int(status), "iterations": int(it), "starting_value": float(r0), "convergence_value": float(r),
                "x": joined(per_rank, f"{pc}_{what}_x")}

    worst = 0.0
    for what in ("zero", "random", "max_it"):
        ref = RC.outer_case(name, pc, what)[1]
        assert ref.iterations == (R.OUTER_MAX_IT if what == "max_it" else R.OUTER_K)
        r = result(what)
        outer_check(r, ref, ("layout_outer", n_ranks, pc, what))
        worst = max(worst, float(np.abs(r["x"] - ref.x).max() / (RC.x_tolerance(name) * np.abs(ref.x).max())))
    r = result("b0")
    assert (r["status"], r["iterations"], r["starting_value"], r["convergence_value"]) == (C.OK, 0, 0.0, 0.0) and not r["x"].any()
    for res in per_rank:
        check_info(res["info"], n_ranks, False)
    say(f"outer CG ({pc}) on the hybrid layout on {n_ranks} ranks", x=worst)
