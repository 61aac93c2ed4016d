"""The reductions behind every printed norm and every CG scalar (dot_partial_kernel, norms_partial_kernel,
reduce_final_kernel, block_sum / block_max) and the vec_* kernels, through gmg_vec_*: integer-valued data make dot, l1,
l2^2 and linf exact in any summation order, so they are compared with ==, at sizes on both sides of the wavefront, the
workgroup and the grid stride (2048 workgroups of 256 threads = 524 288 elements; the 1.93 M-DoF vector is four strides)."""
import math

import numpy as np
import pytest

from gpu_util import capi
from oracle import gmg_oracle as go
from oracle import step50_oracle as so

pytestmark = pytest.mark.gpu
STRIDE = 2048 * 256
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, STRIDE - 1, STRIDE, STRIDE + 1, 1048579, 1930000]
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    c = capi().Context(1)
    yield c
    c.close()


def integers(n):
    i = np.arange(n)
    return ((i % 251) + 1).astype(float), ((i % 13) - 6).astype(float)


def exact_norms(a):
    """l1, l2^2, linf of integer-valued data as Python integers"""
    v = a.astype(np.int64)
    return int(np.abs(v).sum()), int((v * v).sum()), int(np.abs(v).max()) if len(v) else 0


def check_exact(ctx, a, b):
    x, y = ctx.vector(len(a), a), ctx.vector(len(b), b)
    try:
        dot = int((a.astype(np.int64) * b.astype(np.int64)).sum())
        l1, l2sq, linf = exact_norms(a)
        assert l2sq < 2 ** 53 and abs(dot) < 2 ** 53
        assert ctx.dot(x, y) == float(dot)
        g1, g2, gi = ctx.norms(x)
        assert g1 == float(l1) and gi == float(linf)
        assert g2 == math.sqrt(float(l2sq))  # the square root of an exact sum, correctly rounded on the host
        assert ctx.all_zero(x) == (not a.any())
    finally:
        x.free(); y.free()


@pytest.mark.parametrize("n", SIZES)
def test_exact_sums(ctx, n):
    a, b = integers(n)
    check_exact(ctx, a, b)
    for where in (0, n - 1, STRIDE):  # one marker that no other element can hide: dropped or counted twice shows
        if 0 <= where < n:
            am = a.copy()
            am[where] = 2.0 ** 20
            bm = b.copy()
            bm[where] = 2.0 ** 20  # the product is the 2^40 marker
            check_exact(ctx, am, bm)
            am[where] = -2.0 ** 25
            check_exact(ctx, am, np.ones(n))


@pytest.mark.parametrize("n", [1000, STRIDE + 1, 1930000])
def test_rounded_sums_within_the_bound(ctx, n):
    """Gaussian data and a cancelling dot product: |got - exact| <= n u sum|x_i y_i| (any summation order; fsum is exact)"""
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    c = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 + 1e-9 * rng.standard_normal(n))  # neighbours nearly cancel
    x, y = ctx.vector(n, a), ctx.vector(n, b)
    pc = (np.abs(a) + 3.0) * c
    z, w = ctx.vector(n, pc), ctx.vector(n, np.ones(n))
    try:
        for p, q_, pa, qa in ((x, y, a, b), (z, w, pc, np.ones(n))):
            exact, mag = math.fsum(pa * qa), math.fsum(np.abs(pa * qa))
            got = ctx.dot(p, q_)
            # the products are rounded once more than fsum's inputs: (n + 1) u
            print(f"dot n {n}: error / bound {abs(got - exact) / ((n + 1) * U * mag):.2e}, |exact| / sum|.| {abs(exact) / mag:.1e}")
            assert abs(got - exact) <= (n + 1) * U * mag
        l1, l2, li = ctx.norms(x)
        assert abs(l1 - math.fsum(np.abs(a))) <= n * U * math.fsum(np.abs(a))
        assert abs(l2 - math.sqrt(math.fsum(a * a))) <= (n / 2 + 2) * U * math.sqrt(math.fsum(a * a))
        assert li == np.abs(a).max()
    finally:
        for v in (x, y, z, w):
            v.free()


def test_no_stale_partials(ctx):
    """large and small calls alternate on one context: a partial of the larger call must not enter the smaller one"""
    big, small = 1048579, 65
    ab, bb = integers(big)
    as_, bs = integers(small)
    as_, bs = as_ + 1000.0, bs - 50.0
    X, Y, x, y = ctx.vector(big, ab), ctx.vector(big, bb), ctx.vector(small, as_), ctx.vector(small, bs)
    try:
        want_big = (float(int((ab * bb).sum())), *[float(v) for v in exact_norms(ab)])
        want_small = (float(int((as_ * bs).sum())), *[float(v) for v in exact_norms(as_)])
        for k in range(50):
            for (p, q_, want) in ((X, Y, want_big), (x, y, want_small)) if k % 2 == 0 else ((x, y, want_small), (X, Y, want_big)):
                if k % 3:
                    assert ctx.dot(p, q_) == want[0]
                l1, l2, li = ctx.norms(p)
                assert (l1, l2, li) == (want[1], math.sqrt(want[2]), want[3])
                assert ctx.dot(p, q_) == want[0]
    finally:
        for v in (X, Y, x, y):
            v.free()


@pytest.mark.parametrize("n", [1, 64, 257, STRIDE + 1])
def test_all_zero(ctx, n):
    x = ctx.vector(n, np.full(n, -0.0))
    try:
        assert ctx.all_zero(x)  # -0.0 is zero
        ctx.set_zero(x)
        assert ctx.all_zero(x)
        for value in (5e-324, np.nan, -1.0):
            for where in {0, n - 1, n // 2}:
                a = np.zeros(n)
                a[where] = value
                x.upload(a)
                assert not ctx.all_zero(x), (value, where)
    finally:
        x.free()


@pytest.mark.parametrize("n", SIZES)
def test_vector_updates_bitwise(ctx, n):
    rng = np.random.default_rng(n + 1)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    x, y = ctx.vector(n, a), ctx.vector(n, b)
    try:
        ctx.add(y, 0.37, x)
        r = b + 0.37 * a
        assert np.array_equal(y.download(), r)
        ctx.sadd(y, -1.25, 3.0, x)
        r = -1.25 * r + 3.0 * a
        assert np.array_equal(y.download(), r)
        ctx.equ(y, -0.3, x)
        assert np.array_equal(y.download(), -0.3 * a)
        # x aliasing y
        ctx.add(x, 0.37, x)
        r = a + 0.37 * a
        assert np.array_equal(x.download(), r)
        ctx.sadd(x, -1.25, 3.0, x)
        r = -1.25 * r + 3.0 * r
        assert np.array_equal(x.download(), r)
        ctx.equ(x, 7.0, x)
        assert np.array_equal(x.download(), 7.0 * r)
        assert np.array_equal(y.download(), -0.3 * a)  # the neighbour allocation is untouched
    finally:
        x.free(); y.free()


def test_jacobi_preconditioner_bitwise():
    hier = so.build_uniform_hierarchy(3, 0.0, 1.0, 4, problem="Step16")
    c = capi().Context(len(hier.level_matrices))
    try:
        c.load_hierarchy(hier)
        n = hier.system_matrix.n_rows
        src = np.random.default_rng(4).standard_normal(n)
        vs, vd = c.vector(n, src), c.vector(n)
        c.precondition_jacobi(0.6, vd, vs)
        assert np.array_equal(vd.download(), go.OracleMG(hier).precondition_jacobi(src))
    finally:
        c.close()
