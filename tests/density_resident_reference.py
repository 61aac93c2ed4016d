"""Cases and references for gmg_charge_density_resident and gmg_get_resident_cell_geometry, shared by
tests/test_density_resident_cpu.py and tests/test_gpu_density_resident.py.  Written from the comment on the entry in
include/gmg_coulomb.h, not from csrc/gmg_density.hpp.  Plain helper: no fixtures, no tests; everything is computed once.

Geometry.  Two restatements over numpy integers and fp64, both a rounded product followed by a rounded sum:
  geometry_from_tables   the header's formulas on the tables of tests/mesh_tables_reference.py (cell_level and the vertex key of
                         a cell's first DoF);
  geometry_from_forest   the driver's formulas (Forest::cell_origin and the loop of compute_charge_densities) on the integer
                         coordinates of the forest's active cells, level by level in index order.
Densities.  The G dict that rhs_reference.density_numpy / density_mp take is built from that geometry with root_h = h0, so
the bounds derived in tests/rhs_reference.py are the tolerance: no new number.

Atoms.  atoms_reference.gas, scaled into a cube of 3 root cells' edge around the centre of the forest's box (where the
forests are refined, and off the lattice); cutoff = 1.2 h0 and r_c = cutoff / 3.5.  The roots in the middle then have most
atoms on their lists, the roots at the box's corners -- more than the cutoff away from every atom -- none."""
import functools

import numpy as np

import atoms_reference as ar
import mesh_tables_cases as mc
import rhs_reference as rr

KEY_BITS, KEY_SHIFT = 21, 12
MP_SAMPLES = 48  # outputs of the mpmath tier per case (a list may hold 1000 atoms)

#  (forest of tests/mesh_tables_cases.py, atoms, nq): every atom count and every nq once, nq = 8 with every forest
CASES = [("A3", 1000, 8), ("B3", 65, 8), ("G8-c2", 1000, 8), ("A3", 0, 1), ("B3", 1, 27), ("G8-c2", 65, 64), ("A3", 65, 125)]
PARAMS = [(f, n, nq, l) for f, n, nq in CASES for l in (0, 1)]
SEED = {0: 11, 1: 12, 65: 13, 1000: 14}


def active_cells(fc):
    """(level [n], integer coordinates [n, 3]) of the forest's active cells, level by level in index order"""
    lp = np.asarray(fc.level_ptr)
    level_of = np.repeat(np.arange(len(lp) - 1), np.diff(lp))
    act = np.asarray(fc.cell_first_child) < 0
    return level_of[act].astype(np.int64), np.asarray(fc.cell_coord, dtype=np.int64).reshape(-1, 3)[act]


def _geometry(level, c, origin, h0):
    h = h0 / 2.0 ** level
    cell_lo = origin + h[:, None] * c.astype(np.float64)
    root_lo = origin + h0 * (c >> level[:, None]).astype(np.float64)
    return cell_lo, h, root_lo


def geometry_from_forest(fc, origin, h0):
    level, c = active_cells(fc)
    return _geometry(level, c, origin, h0)


def geometry_from_tables(t, origin, h0):
    """t: cell_dofs [n_cells, 8], cell_level, vertex_of_dof as gmg_build_mesh_tables leaves them (or mtr.build's lists)"""
    level = np.asarray(t.cell_level, dtype=np.int64)
    first = np.asarray(t.cell_dofs, dtype=np.int64).reshape(-1, 8)[:, 0]
    key = np.asarray(t.vertex_of_dof, dtype=np.uint64)[first]
    c = np.stack([((key >> np.uint64(KEY_BITS * d)) & np.uint64(0x1fffff)).astype(np.int64) for d in range(3)], 1) >> (KEY_SHIFT - level)[:, None]
    return _geometry(level, c, origin, h0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def atoms(forest, n):
    """(x [n, 3], q [n], r_c, cutoff) for a forest: the gas of atoms_reference, scaled into the middle of the box"""
    s = mc.case(forest)
    h0, n0 = s.h0, int(s.fc.n0[0])
    cutoff = 1.2 * h0
    r_c = cutoff / 3.5
    if n == 0:
        return np.zeros((0, 3)), np.zeros(0), r_c, cutoff
    x, q, _ = ar.gas(SEED[n], n, 1.0)
    u = (x - ar.LO) / float(max(n, 2)) ** (1.0 / 3.0)   # the generator's box [0, L)^3 -> [0, 1)^3
    return s.origin + h0 * (0.5 * n0 - 1.5 + 3.0 * u), q, r_c, cutoff


@functools.lru_cache(maxsize=None)
def geometry(forest, n, nq):
    """the G dict of rhs_reference for a case"""
    s = mc.case(forest)
    lo, h, rlo = geometry_from_forest(s.fc, s.origin, s.h0)
    x, q, r_c, cutoff = atoms(forest, n)
    qp = np.random.default_rng(100 + nq).uniform(0.0, 1.0, (nq, 3))
    return dict(x=x, q=q, r_c=r_c, cutoff=cutoff, root_h=s.h0, cell_lo=lo, cell_h=h, root_lo=rlo, qp=qp, outside=np.zeros(len(h), bool),
                origin=s.origin, h0=s.h0)


@functools.lru_cache(maxsize=None)
def reference(forest, n, nq, use_lists):
    """what rr.check_density takes: both tiers, the mpmath one on MP_SAMPLES outputs"""
    G = geometry(forest, n, nq)
    idx = rr.sample(len(G["cell_h"]) * nq, seed=3, count=MP_SAMPLES)
    return dict(G=G, idx=idx, np=rr.density_numpy(G, use_lists), mp=rr.density_mp(G, use_lists, idx))


def name(forest, n, nq):
    return f"{forest}-n{n}-nq{nq}"
