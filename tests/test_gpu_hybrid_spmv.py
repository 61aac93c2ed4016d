"""The hybrid layout of an operator the SELL rule refuses as a whole: y = A x bit for bit against the
oracle's CSR product and against the library with option disable_hybrid, on the shapes where the layout can go wrong, and the
layout each operator is reported to get (the debug_upload line)."""
import types

import numpy as np
import pytest

from gpu_util import capi, pkg
from oracle import gmg_oracle as go

pytestmark = pytest.mark.gpu

STENCIL = np.array(sorted(dz * 100 + dy * 10 + dx for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)))
FEW = np.array([-0.75, -0.5, -0.25, -0.125, 0.0625, 0.125, 0.25, 0.5, 1.0, 1.5, 2.0, 2.6666666666666665, 1.0 / 3.0, -1.0 / 3.0,
                1.0 / 6.0, -1.0 / 6.0, 1.0 / 12.0, -1.0 / 12.0, 4.0 / 3.0, -0.0])


def csr(rows, n_cols):
    """rows: list of (columns ascending, values)"""
    rp = np.zeros(len(rows) + 1, dtype=np.int64)
    for i, (c, _) in enumerate(rows):
        rp[i + 1] = rp[i] + len(c)
    col = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows]) if rp[-1] else np.zeros(0, dtype=np.int32)
    val = np.concatenate([np.asarray(v, dtype=np.float64) for _, v in rows]) if rp[-1] else np.zeros(0)
    return types.SimpleNamespace(n_rows=len(rows), n_cols=n_cols, rowptr=rp, col=col, val=val, nnz=int(rp[-1]))


def banded(n, wide_rows=(), empty_rows=(), shifted_slices=(), few_regular=True, few_wide=True, seed=0):
    """27 entries per row at row + STENCIL (clipped at the ends: the first and last two slices come out irregular by
    themselves); `wide_rows` get 84 entries; rows of `shifted_slices` with an odd number take their last nine columns 200
    further out (36 offsets in the slice: no column pattern, columns from the stream); values from FEW or all distinct."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        if i in empty_rows:
            rows.append(([], []))
            continue
        off = STENCIL.copy()
        if i // 64 in shifted_slices and i % 2:
            off[18:] += 200
        c = i + off
        c = c[(c >= 0) & (c < n)]
        wide = i in wide_rows
        if wide:
            extra = rng.choice(np.setdiff1d(np.arange(n), c), size=84 - len(c), replace=False)
            c = np.sort(np.concatenate([c, extra]))
        few = few_wide if wide else few_regular
        v = rng.choice(FEW, size=len(c)) if few else rng.standard_normal(len(c))
        rows.append((c, v))
    return csr(rows, n)


def product(m, capfd, expect_layout, seed=1):
    """y = A x from the library with the hybrid layout allowed and refused, and the layout line of the upload"""
    x = np.random.default_rng(seed).standard_normal(m.n_cols)
    c = capi().Context(1)
    try:
        c.set_option("debug_upload", 1)
        capfd.readouterr()
        c.set_system_matrix(m)
        err = capfd.readouterr().err
        c.set_option("debug_upload", 0)
        layouts = [ln.split("layout", 1)[1].split()[0].rstrip(":") for ln in err.splitlines() if "[gmg]   layout" in ln]
        assert layouts == [expect_layout], err
        vx, vy = c.vector(m.n_cols, x), c.vector(m.n_rows)
        got = {}
        for key, two in ((0, 0), (1, 0), (0, 1)):
            c.set_option("disable_hybrid", key)
            c.set_option("hybrid_two_launches", two)  # (the measurement variant: tiles and slices as two kernels)
            vy.upload(np.full(m.n_rows, np.nan))
            c.spmv(capi().SYSTEM, vy, vx)
            got[key, two] = vy.download()
    finally:
        c.close()
    ref = go.spmv(m, x)
    assert np.array_equal(got[1, 0], ref)  # (the CSR row-window kernel, as before)
    assert np.array_equal(got[0, 0], ref)
    assert np.array_equal(got[0, 1], ref)
    return err


@pytest.mark.parametrize("name,kw", [
    ("wide row in the middle of slice 3", dict(n=1088, wide_rows=(3 * 64 + 32,))),
    ("wide rows in the first and the last slice", dict(n=1088, wide_rows=(5, 1088 - 7))),
    ("partial last slice", dict(n=1100, wide_rows=(3 * 64 + 32,))),
    ("empty rows, an empty slice, streamed columns", dict(n=1088, wide_rows=(3 * 64 + 32, 9 * 64), empty_rows=tuple(range(400, 404)) + tuple(range(640, 704)),
                                                          shifted_slices=(5, 6, 7))),
    ("> 256 values overall, <= 256 in the regular slices", dict(n=1088, wide_rows=tuple(range(3 * 64 + 30, 3 * 64 + 36)), few_wide=False)),
    ("> 256 values in the regular slices", dict(n=1088, wide_rows=(3 * 64 + 32,), few_regular=False, shifted_slices=(6,))),
])
def test_hybrid_product_bit_exact(capfd, name, kw):
    m = banded(**kw)
    err = product(m, capfd, "hybrid")
    want_val8 = 0 if name.startswith("> 256 values in the regular") else 1
    assert f"val8 {want_val8}" in err, err


def test_all_regular_and_all_irregular_keep_todays_layouts(capfd):
    n = 1088
    rng = np.random.default_rng(3)
    regular = csr([(np.unique((i * 7 + 13 * np.arange(8) + np.arange(8) ** 2) % n), rng.choice(FEW, size=8)) for i in range(n)], n)
    assert np.all(np.diff(regular.rowptr) == 8)
    product(regular, capfd, "sell")
    rows = []
    for i in range(n):
        c = np.arange(i - i % 64, i - i % 64 + 64) if i % 64 == 17 else np.array([i])
        rows.append((c, rng.standard_normal(len(c))))
    product(csr(rows, n), capfd, "csr")


def test_real_system_matrix_with_hanging_nodes(capfd):
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=1, mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous",
                             cycles=3, r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="Jacobi"))
    try:
        p.set_nacl_atoms(1)
        for cycle in range(3):
            p.run_cycle(cycle, on_device=True)
        m = p.hierarchy().system_matrix
    finally:
        p.close()
    w = np.diff(np.asarray(m.rowptr))
    assert w.max() > 32 and np.median(w) == 27  # hanging-node rows among lattice rows
    product(m, capfd, "hybrid")
