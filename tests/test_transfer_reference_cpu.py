"""CPU checks of tests/transfer_reference.py and tests/transfer_cases.py, the reference that
tests/test_gpu_transfer_reference.py holds gmg_build_transfer to: its two evaluators agree array for array, the cell-by-cell
one equals the host-built operators on the driver's meshes, the operators have the structure of a Q1 embedding, every case
reaches the edge it is there for, the application bound is sound, and every seeded mistake in the reference is noticed by
exactly the cases named here."""
import numpy as np
import pytest

import transfer_cases as TC
import transfer_reference as TR

SMALL = [n for n in TC.NAMES if TC.SIZES[n][1] <= TC.DENSE_LIMIT]


def _table_size(n):
    """the header's rule of the hash table: the first power of two that is at least 2 n and at least 1024"""
    t = 1024
    while t < 2 * n:
        t *= 2
    return t


def _coords(keys, dim):
    return np.stack([(keys >> np.uint64(21 * d)) & np.uint64(0x1FFFFF) for d in range(3)], axis=1).astype(np.int64)


@pytest.mark.parametrize("name", SMALL)
def test_evaluators_agree(name):
    c = TC.case(name)
    assert c.dense is not None
    assert TR.same(c.dense[0], c.P), name
    assert TR.same(c.dense[1], c.Pt), name


def test_the_dense_evaluator_runs_on_every_case_it_can():
    assert set(TC.NAMES) - set(SMALL) == set(TC.SCAN)
    assert all(TC.case(n).dense is None for n in TC.SCAN)


@pytest.mark.parametrize("name", list(TC.MESH))
def test_reference_equals_host(name):
    from test_gpu_transfer import _transpose_stable

    c = TC.case(name)
    H = c.host_P
    assert (H.n_rows, H.n_cols, H.nnz) == (c.P.n_rows, c.P.n_cols, c.P.nnz)
    assert np.array_equal(H.rowptr, c.P.rowptr) and np.array_equal(H.col, c.P.col) and np.array_equal(H.val, c.P.val)
    trp, tcol, tval = _transpose_stable(H)
    assert np.array_equal(trp, c.Pt.rowptr) and np.array_equal(tcol, c.Pt.col) and np.array_equal(tval, c.Pt.val)
    assert not c.random_numbering


@pytest.mark.parametrize("name", TC.NAMES)
def test_structure(name):
    c = TC.case(name)
    P, Pt = c.P, c.Pt
    assert P.rowptr.dtype == Pt.rowptr.dtype == np.int64 and P.col.dtype == Pt.col.dtype == np.int32 and P.val.dtype == Pt.val.dtype == np.float64
    assert (P.n_rows, P.n_cols, Pt.n_rows, Pt.n_cols) == (c.n_fine, c.n_coarse, c.n_coarse, c.n_fine) and P.nnz == Pt.nnz
    allowed = (1.0, 0.5, 0.25, 0.125) if c.dim == 3 else (1.0, 0.5, 0.25)
    assert np.all(np.isin(P.val, allowed)) and np.all(np.isin(Pt.val, allowed))
    for m in (P, Pt):   # strictly ascending inside every row
        inner = np.ones(m.nnz, dtype=bool)
        inner[m.rowptr[:-1][np.diff(m.rowptr) > 0]] = False
        assert np.all(np.diff(m.col.astype(np.int64))[inner[1:]] > 0)
    assert not np.any(c.coarse_boundary[P.col])   # no boundary column
    # a fine vertex has 2^(directions in which it lies between two coarse vertices) parents; where none was dropped the row
    # sums to exactly 1, and a row that lost a parent to the boundary sums to less
    xf = _coords(c.fine_vertex, c.dim)[:, :c.dim]
    parents = 1 << np.sum(xf % (2 * c.fine_spacing) != 0, axis=1)
    count = np.diff(P.rowptr)
    total = np.zeros(c.n_fine)
    np.add.at(total, np.repeat(np.arange(c.n_fine), count), P.val)
    assert np.all(count <= parents)
    assert np.all(total[count == parents] == 1.0) and np.all(total[count < parents] < 1.0)
    if P.nnz and name != "centre-3d":
        assert np.any(count == parents)


def test_cases_reach_their_edges():
    C = TC.case
    for n in ("one-cell-2d", "one-cell-3d"):
        assert C(n).P.nnz == C(n).Pt.nnz == 0 and np.all(C(n).coarse_boundary == 1)
    c = C("centre-3d")
    assert int(np.sum(c.coarse_boundary == 0)) == 1 and int(np.diff(c.Pt.rowptr).max()) == 27 and np.any(np.diff(c.P.rowptr) == 0)
    assert 0.25 < C("L-3d-drawn").coarse_boundary.mean() < 0.35 and not np.array_equal(C("L-3d-drawn").coarse_boundary, C("L-3d").coarse_boundary)
    assert int(np.sum(np.diff(C("two-cells-3d").Pt.rowptr) == 0)) > C("two-cells-3d").n_coarse // 2
    for n in TC.TOP_OF_RANGE:   # bit 20 of every field; the largest coordinate is the largest multiple of 2 fine_spacing below 2^21
        c = C(n)
        x = _coords(np.concatenate([c.coarse_vertex, c.fine_vertex]), c.dim)[:, :c.dim]
        assert np.all(x.max(axis=0) == (1 << 21) - 2 * c.fine_spacing) and np.all(x.min(axis=0) > 0)
        assert np.all(x >> 20 == 1)
        if c.dim == 3:
            assert int(c.coarse_vertex.max() >> np.uint64(62)) == 1   # the highest bit the key has
    for n in ("origin-L-3d", "origin-checker-2d"):
        c = C(n)
        assert np.all(_coords(c.coarse_vertex, c.dim)[:, :c.dim].min(axis=0) == 0)
        interior_at_0 = (c.coarse_boundary == 0) & np.any(_coords(c.coarse_vertex, c.dim)[:, :c.dim] == 0, axis=1)
        assert not np.any(interior_at_0)   # geometric flags: every row of the transpose at coordinate 0 is empty by its flag ...
    assert [C(n).fine_spacing for n in ("spacing-1", "spacing-4096", "spacing-2p18")] == [1, 4096, 1 << 18]
    x = _coords(C("spacing-2p18").coarse_vertex, 3)
    assert x.max() == 3 << 19 and x.max() + (2 << 18) == 1 << 21   # one more coarse vertex would not fit the field
    assert (_table_size(C("load-512").n_coarse), _table_size(C("load-513").n_coarse)) == (1024, 2048) and 2 * C("load-512").n_coarse == 1024
    assert [C(n).n_coarse for n in ("scan-c16384", "scan-c16385")] == [TR.SCAN_PASS, TR.SCAN_PASS + 1]
    assert [C(n).n_fine for n in ("scan-f16384", "scan-f16385", "scan-f32769")] == [TR.SCAN_PASS, TR.SCAN_PASS + 1, 2 * TR.SCAN_PASS + 1]
    assert max(C(n).n_fine for n in TC.NAMES) == C("scan-c16384").n_fine == 65025


def test_drawn_flags_reach_coordinate_zero():
    """... so origin-L-3d-drawn carries what geometric flags cannot: interior coarse DoFs at coordinate 0 with entries, whose
    rows of the transpose would look for fine vertices at negative coordinates"""
    c = TC.case("origin-L-3d-drawn")
    x = _coords(c.coarse_vertex, 3)
    assert np.all(x.min(axis=0) == 0)
    for d in range(3):
        assert np.any((x[:, d] == 0) & (c.coarse_boundary == 0) & (np.diff(c.Pt.rowptr) > 0)), d


@pytest.mark.parametrize("name", TC.NAMES)
def test_application_bound_is_sound(name):
    """the fp64 sum in stored order stays within the bound of the longdouble value, and the bound is no blanket: it is a few
    units of the row's own magnitude"""
    c = TC.case(name)
    x, r, dst0 = TC.vectors(name)
    for v in (x, r, dst0):
        mag = np.abs(v)
        assert mag.max() / mag.min() > 1e5 and np.any(v < 0) and np.any(v > 0)
    y, b = TR.apply_reference(c.P, x)
    assert TR.error_ratio(TR.sequential(c.P, x), y, b) <= 1.0
    assert np.all(b[np.diff(c.P.rowptr) == 0] == 0.0)
    z, bz = TR.apply_reference(c.Pt, r, dst0)
    assert TR.error_ratio(TR.sequential(c.Pt, r, dst0), z, bz) <= 1.0
    assert np.all(bz > 0) and np.all(bz <= 28 * 2.0 ** -52 * (np.abs(dst0) + 27 * np.abs(r).max()))
    # an error of one part in 10^12 in one entry is outside the bound (rows of at most 27 entries: gamma_28 = 3.1e-15)
    if c.P.nnz:
        i = int(np.argmax(np.abs(y)))
        bad = TR.sequential(c.P, x)
        bad[i] *= 1.0 + 1e-12
        assert TR.error_ratio(bad, y, b) > 1.0


# which cases notice which seeded mistake (from_cells(..., mistake=...) against the reference, array for array)
_RANDOM = tuple(n for n in TC.NAMES if n not in TC.MESH)
_MULTI = tuple(n for n in _RANDOM if n not in ("one-cell-2d", "one-cell-3d"))   # some row of P^T has two entries or more
NOTICED = {
    # the driver's finer levels (mesh-A3-1, mesh-S2) have no boundary DoF next to a refined cell
    "boundary-kept": tuple(n for n in TC.NAMES if n not in ("mesh-A3-1", "mesh-S2")),
    # every 2D case with an entry
    "weights-3d": ("checker-2d", "top-checker-2d", "origin-checker-2d", "load-512", "load-513") + TC.SCAN + ("mesh-S2",),
    # every randomly numbered case with a row of two entries (centre-3d has one column), and the driver's first-touch levels:
    # first touch is no coordinate order either.  Level 0 of A3 is numbered lexicographically, which IS the coordinate order
    # (mesh-A3-0 does not notice): only a numbering that is not the driver's level-0 order tells the two sorts apart
    "row-by-coordinate": tuple(n for n in _MULTI if n != "centre-3d") + ("mesh-A3-1", "mesh-S2"),
    "transpose-by-coordinate": _MULTI + ("mesh-A3-0", "mesh-A3-1", "mesh-S2"),
    # no well-formed mesh can: see test_an_absent_parent_needs_an_ill_formed_mesh
    "absent-parent": (),
    # top-of-range, and spacing-2p18, whose 3 cells of 2^19 span 3 * 2^19 > 2^20 wherever they are put
    "key-20-bits": TC.TOP_OF_RANGE + ("spacing-2p18",),
    "rowptr-restart": TC.SCAN,
}


@pytest.mark.parametrize("mistake", TR.MISTAKES)
def test_seeded_mistakes_are_noticed_by_the_named_cases(mistake):
    seen = []
    for name in TC.NAMES:
        c = TC.case(name)
        P, Pt = TR.from_cells(c.dim, c.coarse_vertex, c.coarse_boundary, c.fine_vertex, c.cells, c.fine_spacing, mistake=mistake)
        if not (TR.same(P, c.P) and TR.same(Pt, c.Pt)):
            seen.append(name)
    assert sorted(seen) == sorted(NOTICED[mistake]), (mistake, seen)
    if mistake != "absent-parent":
        assert seen


def test_the_ordering_mistakes_need_a_numbering_that_is_not_lexicographic():
    """the two ordering mistakes are invisible on a level numbered in coordinate order, which is what the driver's level 0
    is: L-3d renumbered that way is the reference again under both"""
    c = TC.case("L-3d")
    co, fo = np.argsort(c.coarse_vertex), np.argsort(c.fine_vertex)
    args = (3, c.coarse_vertex[co], c.coarse_boundary[co], c.fine_vertex[fo], c.cells, c.fine_spacing)
    ref = TR.from_cells(*args)
    for mistake in ("row-by-coordinate", "transpose-by-coordinate"):
        got = TR.from_cells(*args, mistake=mistake)
        assert TR.same(got[0], ref[0]) and TR.same(got[1], ref[1])
        assert mistake in NOTICED and "L-3d" in NOTICED[mistake]


def test_an_absent_parent_needs_an_ill_formed_mesh():
    """Every parent of a fine vertex is a vertex of the refined cell whose child the fine vertex belongs to, and a level holds
    every vertex of its cells: on a well-formed pair of levels no parent is absent, and the mistake of giving an absent parent
    an entry changes nothing (NOTICED["absent-parent"] is empty; the contract leaves ill-formed meshes open, so no case is one).
    That the seeded mistake is live all the same: with one interior coarse vertex struck from the table it adds entries."""
    c = TC.case("centre-3d")
    keep = c.coarse_boundary == 1
    assert int(np.sum(~keep)) == 1
    with pytest.raises(ValueError):
        TR.from_cells(3, c.coarse_vertex[keep], c.coarse_boundary[keep], c.fine_vertex, c.cells, c.fine_spacing)
    P, _ = TR.from_cells(3, c.coarse_vertex[keep], c.coarse_boundary[keep] * 0, c.fine_vertex, c.cells, c.fine_spacing, mistake="absent-parent")
    Q, _ = TR.from_cells(3, c.coarse_vertex[keep], c.coarse_boundary[keep] * 0, c.fine_vertex, c.cells, c.fine_spacing, mistake="key-20-bits")
    assert P.nnz > Q.nnz   # (key-20-bits changes no key here and drops what it does not find)
