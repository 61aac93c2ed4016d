"""gmg_build_transfer (csrc/gmg_transfer.hpp) against the geometric definition of tests/transfer_reference.py on the cases of
tests/transfer_cases.py: the device's CSR arrays of P and of its transpose bit for bit, their
application within the derived bound and equal to the sequential sum, repeatability, rebuilds on a live context, the stats
and the refusals.  tests/test_transfer_reference_cpu.py proves that the reference's two evaluators agree and that every seeded
mistake in it is noticed on these cases.  All device work goes through capi.Context, one Context(2) per test, set up in the
driver's order: level matrices (diagonal ones of the two sizes), then the transfer."""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import transfer_cases as TC
import transfer_reference as TR
from gpu_util import capi
from oracle import gmg_oracle as go

pytestmark = pytest.mark.gpu


def _diagonal(n):
    return SimpleNamespace(n_rows=n, n_cols=n, nnz=n, rowptr=np.arange(n + 1, dtype=np.int64), col=np.arange(n, dtype=np.int32), val=np.full(n, 2.0))


def _level_matrices(ctx, n_coarse, n_fine):
    ctx.set_level_matrix(0, _diagonal(n_coarse))
    ctx.set_level_matrix(1, _diagonal(n_fine))


def _build(ctx, c):
    return ctx.build_transfer(0, c.dim, c.coarse_vertex, c.coarse_boundary, c.fine_vertex, c.fine_spacing)


def _same_arrays(ctx, c, what=""):
    for transposed, ref in ((False, c.P), (True, c.Pt)):
        dev = ctx.get_transfer(0, transposed)
        assert (dev.n_rows, dev.n_cols, dev.nnz) == (ref.n_rows, ref.n_cols, ref.nnz), (what, c.name, transposed, dev.n_rows, dev.n_cols, dev.nnz)
        assert len(dev.rowptr) == ref.n_rows + 1 and len(dev.col) == len(dev.val) == ref.nnz
        assert np.array_equal(dev.rowptr, ref.rowptr), (what, c.name, transposed, "rowptr")
        assert np.array_equal(dev.col, ref.col), (what, c.name, transposed, "col")
        assert np.array_equal(dev.val.view(np.uint64), ref.val.view(np.uint64)), (what, c.name, transposed, "val")


def _apply(ctx, c, what=""):
    """prolongate into NaN and restrict_and_add onto a non-zero dst: within the bound of the longdouble value, and the bits of
    the sequential sum; returns the worst error-to-bound ratio"""
    x, r, dst0 = TC.vectors(c.name)
    dx, dr = ctx.vector(c.n_coarse, x), ctx.vector(c.n_fine, r)
    fine = ctx.vector(c.n_fine, np.full(c.n_fine, np.nan))
    ctx.prolongate(0, fine, dx)
    got = fine.download()
    y, bound = TR.apply_reference(c.P, x)
    ratio_p = TR.error_ratio(got, y, bound)
    assert not np.any(np.isnan(got)), (what, c.name, "a row of P x was not written")
    assert ratio_p <= 1.0, (what, c.name, "prolongate", ratio_p)
    assert np.array_equal(got, go.spmv(c.P, x)), (what, c.name, "prolongate is not the sequential sum")
    coarse = ctx.vector(c.n_coarse, dst0)
    ctx.restrict_and_add(0, coarse, dr)
    got = coarse.download()
    z, bound = TR.apply_reference(c.Pt, r, dst0)
    ratio_r = TR.error_ratio(got, z, bound)
    assert ratio_r <= 1.0, (what, c.name, "restrict_and_add", ratio_r)
    assert np.array_equal(got, go.spmv_transpose(c.P, r, y0=dst0)), (what, c.name, "restrict_and_add is not the sequential Tvmult")
    if c.P.nnz == 0:
        assert np.all(fine.download() == 0.0) and np.array_equal(got, dst0)
    for v in (dx, dr, fine, coarse):
        v.free()
    return max(ratio_p, ratio_r)


@pytest.mark.parametrize("name", TC.NAMES)
def test_arrays_equal_the_definition(name):
    t0 = time.perf_counter()
    c = TC.case(name)
    ctx = capi().Context(2)
    _level_matrices(ctx, c.n_coarse, c.n_fine)
    ms = _build(ctx, c)
    _same_arrays(ctx, c)
    print(f"[transfer-gpu] arrays {name}: {c.n_coarse} -> {c.n_fine}, nnz {c.P.nnz}, identical; build {ms:.3f} ms, test {time.perf_counter() - t0:.2f} s")
    ctx.close()


@pytest.mark.parametrize("name", TC.NAMES)
def test_application_within_the_bound_and_sequential(name):
    t0 = time.perf_counter()
    c = TC.case(name)
    ctx = capi().Context(2)
    _level_matrices(ctx, c.n_coarse, c.n_fine)
    _build(ctx, c)
    ratio = _apply(ctx, c)
    print(f"[transfer-gpu] application {name}: worst error / bound {ratio:.3f}, test {time.perf_counter() - t0:.2f} s")
    ctx.close()


def test_no_level_matrix_is_needed():
    """on one rank the transfer and both applications stand without level matrices (recorded in DESIGN.md section 31)"""
    c = TC.case("L-3d")
    ctx = capi().Context(2)
    _build(ctx, c)
    _same_arrays(ctx, c)
    print(f"[transfer-gpu] no level matrices L-3d: worst error / bound {_apply(ctx, c):.3f}")
    ctx.close()


def test_repeated_builds_give_the_same_arrays():
    """whichever thread wins a slot of the hash table"""
    ctx = capi().Context(2)
    worst = 0.0
    for name in ("L-3d", "load-512"):
        c = TC.case(name)
        _level_matrices(ctx, c.n_coarse, c.n_fine)
        seen = []
        for _ in range(3):
            _build(ctx, c)
            _same_arrays(ctx, c, "repeat")
            seen.append([ctx.get_transfer(0, t) for t in (False, True)])
        for again in seen[1:]:
            for a, b in zip(seen[0], again):
                assert np.array_equal(a.rowptr, b.rowptr) and np.array_equal(a.col, b.col) and np.array_equal(a.val.view(np.uint64), b.val.view(np.uint64))
        worst = max(worst, _apply(ctx, c, "repeat"))
    print(f"[transfer-gpu] repeatability: 3 builds each of L-3d and load-512 identical; worst error / bound {worst:.3f}")
    ctx.close()


def test_rebuild_on_a_live_context():
    """a smaller device-built transfer over a larger one, a host-given one over that, a device-built one over the host-given:
    after each step the arrays and both applications are that step's"""
    C = capi()
    ctx = C.Context(2)
    worst = 0.0
    steps = (("L-3d", "device"), ("two-cells-3d", "device"), ("checker-2d", "host"), ("centre-3d", "device"))
    for name, how in steps:
        c = TC.case(name)
        _level_matrices(ctx, c.n_coarse, c.n_fine)
        if how == "device":
            _build(ctx, c)
            _same_arrays(ctx, c, "rebuild")
        else:
            ctx.set_prolongation(0, c.P)
            try:   # (a host-given operator may have been given another layout, without a CSR copy)
                _same_arrays(ctx, c, "rebuild, host-given")
            except C.GMGError as e:
                assert e.code == C.ERR_UNSUPPORTED, e
        worst = max(worst, _apply(ctx, c, "rebuild"))
    print(f"[transfer-gpu] rebuild: {' / '.join(n for n, _ in steps)}; worst error / bound {worst:.3f}")
    ctx.close()


def test_build_time_is_counted_and_reset():
    ctx = capi().Context(2)
    assert ctx.stats().build_matrices_ms == 0.0
    total = 0.0
    for name in ("L-3d", "checker-2d", "L-3d"):
        c = TC.case(name)
        _level_matrices(ctx, c.n_coarse, c.n_fine)
        ms = _build(ctx, c)
        assert ms > 0.0
        total += ms
        assert ctx.stats().build_matrices_ms == total
    ctx.reset(2)
    assert ctx.stats().build_matrices_ms == 0.0
    c = TC.case("centre-3d")   # and the context builds again after the reset
    _level_matrices(ctx, c.n_coarse, c.n_fine)
    assert _build(ctx, c) == ctx.stats().build_matrices_ms > 0.0
    _same_arrays(ctx, c, "after reset")
    print(f"[transfer-gpu] stats: three builds {total:.3f} ms counted, 0 after reset")
    ctx.close()


def test_refusals_leave_the_context_usable():
    C = capi()
    ctx = C.Context(2)
    c = TC.case("checker-2d")
    _level_matrices(ctx, c.n_coarse, c.n_fine)
    none64, none8 = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8)
    good = dict(level=0, dim=c.dim, coarse_vertex=c.coarse_vertex, coarse_boundary=c.coarse_boundary, fine_vertex=c.fine_vertex, fine_spacing=c.fine_spacing)
    bad = [dict(level=-1), dict(level=ctx.n_levels - 1), dict(dim=1), dict(dim=4), dict(fine_spacing=0), dict(fine_spacing=3),
           dict(coarse_vertex=none64, coarse_boundary=none8), dict(fine_vertex=none64)]
    worst = 0.0
    for change in bad:
        with pytest.raises(C.GMGError) as e:
            ctx.build_transfer(**{**good, **change})
        assert e.value.code == C.ERR_INVALID, (change.keys(), e.value.code)
        ctx.build_transfer(**good)   # the next valid build still works
        _same_arrays(ctx, c, f"after refusing {sorted(change)}")
        worst = max(worst, _apply(ctx, c, "after a refusal"))
    print(f"[transfer-gpu] refusals: {len(bad)} refused with GMG_ERR_INVALID, each followed by a valid build; worst error / bound {worst:.3f}")
    ctx.close()
