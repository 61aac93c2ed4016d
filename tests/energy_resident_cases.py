"""What tests/test_energy_resident_cpu.py and tests/test_gpu_energy_resident.py share.  Plain helper: no
fixtures, no tests.

node_array(fc): "node array from a forest" as gmg_build_point_locator_resident defines it, in plain numpy.

energy_sums(q, phi, e_short, r_c): the three ascending sums of gmg_electrostatic_energy_resident in plain Python floats (IEEE
fp64, one operation at a time, so no fused multiply-add).

The forests and atom sets of the GPU tests, and the host's point_locator() for every step of tests/refine_cases.py, found by
driving the same families with the steps' own flags (no solve is repeated) -- computed once, left unchanged.

The bound of the short-range sum.  short = sum_i e_i with e_i = 1/2 sum_j t_ij one sequential sum of n_i addends.  As in
tests/atoms_reference.py (u = 2^-53, C_energy(s) = 9 s^2 + 43 the relative error of one addend in units of u):

    |e_i - exact_i| <= b_i = 1/2 u sum_j (n_i + C_energy(s_ij)) |t_ij| + n_i 2^-1022

and the last sum, n addends e_i in sequence, adds at most n u sum_i |e_i| (recursive summation, first order as there):

    |short - exact| <= B = sum_i b_i + n u sum_i |e_i|

b_i and e_i are the reference's (bound_e and e of pair_sums_numpy or pair_sums_mp): nothing the kernels return enters.  Against
the fp64 numpy reference, whose own sum carries the same bound, the distance allowed is B as well: the reference's per-atom
values stand for the exact ones exactly as tests/atoms_reference.py lets them (its two tiers are held to agree within b_i).

The host's short-range sum of postprocess_electrostatic_energy adds the same pairs once each (i < j) instead of twice halved.
With a cutoff it forms per-atom partial sums of at most n_i addends and adds the n partial sums: the same B bounds it.  Without
a cutoff it is ONE sequential sum of all P = n (n - 1) / 2 pairs: |host - exact| <= u sum_pairs (P + C_energy(s)) |t| + P 2^-1022.
A driver run with the key off and one with it on may therefore differ by B + (the host's bound).
"""
import functools
import math
import os
from types import SimpleNamespace

import numpy as np

import atoms_reference as ar
import mesh_tables_cases as mtc
import mesh_tables_reference as mtr
import refine_cases as rc
import refine_reference as rr


# ------------------------------------------------------------------------------------------------ the node array

def node_array(fc):
    """node[k] = level_ptr[l + 1] + first_child[k] for a refined cell k = level_ptr[l] + c, -(active number of k) - 1 otherwise;
    the active number is the count of active cells before k in (level, index) order"""
    first_child = np.asarray(fc.cell_first_child, dtype=np.int64).reshape(-1)
    level_ptr = [int(v) for v in np.asarray(fc.level_ptr).reshape(-1)]
    node = np.zeros(len(first_child), dtype=np.int32)
    seen = 0
    for l in range(fc.n_levels):
        for k in range(level_ptr[l], level_ptr[l + 1]):
            if first_child[k] >= 0:
                node[k] = level_ptr[l + 1] + first_child[k]
            else:
                node[k] = -seen - 1
                seen += 1
    return node


def properties(fc):
    """what a forest offers a wrong kernel: (a root is active, a root is three levels deep beside a shallower one, an inactive
    cell lies between two active ones in index order)"""
    node = node_array(fc)
    level_ptr = [int(v) for v in np.asarray(fc.level_ptr).reshape(-1)]
    n_roots = level_ptr[1] if fc.n_levels else 0
    nch = 1 << fc.dim

    def depth(k):
        return 0 if node[k] < 0 else 1 + max(depth(int(node[k]) + a) for a in range(nch))

    depths = [depth(k) for k in range(n_roots)]
    active = node < 0
    hit = np.flatnonzero(active)
    between = len(hit) >= 2 and bool((~active[hit[0]:hit[-1]]).any())
    return (0 in depths, max(depths, default=0) >= 3 and min(depths, default=0) < 3, between)


# ------------------------------------------------------------------------------------------------ the three sums

def energy_sums(q, phi, e_short, r_c):
    """(short, fe_long, self): each one sequential sum in ascending atom index"""
    short = fe = self_e = 0.0
    denom = math.sqrt(math.pi) * float(r_c)
    for i in range(len(q)):
        qi = float(q[i])
        short += float(e_short[i])
        fe += (0.5 * qi) * float(phi[i])
        self_e += qi * qi / denom
    return short, fe, self_e


def short_bound(ref):
    """B of the docstring from a reference of tests/atoms_reference.py (dict with e and bound_e of every atom)"""
    e, b = np.asarray(ref["e"], float), np.asarray(ref["bound_e"], float)
    return float(b.sum() + len(e) * ar.U * np.abs(e).sum())


def host_short_bound(x, q, r_c, cutoff, ref):
    """the bound of the host's sum (docstring): B with a cutoff, the single sum over all pairs without"""
    if cutoff > 0:
        return short_bound(ref)
    n = len(q)
    P = n * (n - 1) // 2
    total = 0.0
    for i in range(n):
        d = x[i] - x[i + 1:]
        r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        s = r / r_c
        t = np.abs(q[i] * q[i + 1:] * np.vectorize(math.erfc, otypes=[float])(s) / r) if len(r) else np.zeros(0)
        total += float(((P + ar.c_short_energy(s)) * t).sum())
    return ar.U * total + P * ar.TINY


@functools.lru_cache(maxsize=None)
def pair_case(case_id):
    """atoms of a case of tests/atoms_reference.py with BOTH tiers on every atom: namespace(x, q, r_c, cutoff, np, mp)"""
    r_c, cutoff, make = ar.PAIR_CASES[case_id]
    x, q, _ = make()
    return SimpleNamespace(x=x, q=q, r_c=r_c, cutoff=cutoff, np=ar.pair_sums_numpy(x, q, r_c, cutoff), mp=ar.pair_sums_mp(x, q, r_c, cutoff, np.arange(len(q))))


ENERGY_PAIR_CASES = ("gas1-rc0.5-cut0", "gas65-rc0.5-cut0", "gas65-rc0.37-cut2.5", "gas257-rc0.5-cut1.5")


# ------------------------------------------------------------------------------------------------ forests

def _deep():
    """3 x 3 x 3 roots; root 0 refined, its child (1, 1, 1) refined, the level-2 cell (3, 3, 3) refined: root 0 is three levels
    deep, the closure leaves the roots around the vertex (1, 1, 1) shallower, the roots of the far sides stay active"""
    return rr.refined(rr.lattice(3, 3), [(0, 0, 0, 0)], [(1, 1, 1, 1)], [(2, 3, 3, 3)])


def _wide():
    """4 x 4 x 4 roots, the inner 2 x 2 x 2 and a corner root refined, six level-1 cells refined again: about 300 cells"""
    inner = [(0, x, y, z) for z in (1, 2) for y in (1, 2) for x in (1, 2)]
    return rr.refined(rr.lattice(3, 4), inner + [(0, 3, 0, 0)], [(1, 3, 3, 3), (1, 4, 4, 4), (1, 3, 4, 3), (1, 4, 3, 4), (1, 2, 2, 2), (1, 5, 5, 5)])


FORESTS = {"lattice-2": lambda: rr.lattice(3, 2), "edge-3d": mtr.edge_only_3d, "deep": _deep, "wide": _wide}


@functools.lru_cache(maxsize=None)
def forest(name):
    return FORESTS[name]()


GEOMETRY = {"binary": (-0.5, 0.25), "decimal": (-0.375, 0.3)}   # (origin, h0): exact binary fractions, and not


def atom_set(fc, origin, h0, n, seed=3):
    """n atoms (0, 1 or 40) for a 3D forest on the root lattice at origin with cell size h0.  The 40: points given in lattice
    units t, x = origin + h0 t (exact where origin and h0 are binary fractions) -- on a face, an edge and a vertex between
    root 0 and its neighbours (a refinement interface where root 0 is refined), on vertices, edges and faces inside root 0 at
    levels 1 to 3, on the domain boundary and its corners, just outside it (the clamp), one and a half cells outside, exactly at
    the -2 and n0 + 2 thresholds of the far path, far outside; the rest uniform in the box.  No two atoms coincide."""
    n0 = [int(v) for v in fc.n0]
    if n == 0:
        return np.zeros((0, 3)), np.zeros(0)
    rng = np.random.default_rng(seed + n)
    top = [float(v) for v in n0]
    eps = 2.0 ** -30
    inside = lambda d: 0.3 * min(1.0, top[d])
    special = [
        (1.0, 0.3, 0.3), (0.3, 1.0, inside(2)), (1.0, 1.0, 0.3), (1.0, 1.0, min(1.0, top[2])),       # face, face, edge, vertex of root 0
        (0.5, 0.5, 0.5), (0.5, 0.25, 0.3), (0.75, 0.75, 0.75), (0.75, 0.5, 0.6), (0.875, 0.875, 0.875), (0.875, 0.75, 0.8),
        (0.5, 0.5, 0.3), (0.75, 0.3, 0.3), (1.0, 0.5, 0.5), (1.0, 0.75, 0.25), (0.5, 1.0, 0.75),
        (0.0, 0.3, 0.4), (top[0], 0.6, 0.2), (0.3, 0.0, 0.1), (0.4, top[1], 0.3), (0.2, 0.7, 0.0), (0.6, 0.1, top[2]),   # boundary faces
        (0.0, 0.0, 0.0), (top[0], top[1], top[2]), (0.0, top[1], 0.0),                                                  # corners
        (-eps, 0.4, 0.4), (top[0] + eps, 0.9, 0.1), (0.9, -eps, top[2] + eps),                                          # just outside
        (-1.5, 0.5, 0.5), (top[0] + 1.5, 0.2, 0.2), (0.1, 0.1, top[2] + 1.5),                                           # outside, near path
        (-2.0, 0.2, 0.6), (top[0] + 2.0, 0.4, 0.8), (0.7, -2.0 - eps, 0.2),                                             # the thresholds
        (-50.0, 1.0, 0.5), (1.0e6, 0.5, 0.5), (0.5, 0.5, -3.0e9),                                                       # far outside
    ]
    if n == 1:
        t = np.array([special[2]])
    else:
        fill = rng.uniform(0.0, 1.0, (max(n - len(special), 0), 3)) * np.array(top)
        t = np.vstack([np.array(special), fill])[:n]
    xyz = origin + h0 * t
    assert len({tuple(p) for p in xyz.tolist()}) == len(xyz)
    q = rng.choice([-1.0, 1.0], len(xyz)) * rng.uniform(0.5, 1.5, len(xyz))
    return np.ascontiguousarray(xyz), q


# ------------------------------------------------------------------------------------------------ the host's arrays

@functools.lru_cache(maxsize=None)
def _host_nodes(family):
    """per forest of the family's steps (the one that goes into step 0, then every step's new forest): the host's point_locator(),
    the forests reached by refining with the steps' own flags"""
    steps = [rc.step(n) for n in rc.STEPS if n.split(":")[0] == family]
    p, _, _ = mtc._open(family.split("-")[0])
    p.run_cycle(0, on_device=False)
    out = [(p.forest_cells(), p.point_locator())]
    for s in steps:
        p.finish_cycle_with(np.zeros(p.n_dofs()))
        p.refine_with_flags(np.asarray(s.flag, dtype=np.uint8), on_device=False)
        out.append((p.forest_cells(), p.point_locator()))
    p.close()
    return tuple(out)


def host_nodes(name):
    """(forest that went into the step, host node array, new forest, host node array) of a step of tests/refine_cases.py"""
    family, rest = name.split(":")
    c = int(rest.split("->")[0])
    nodes = _host_nodes(family)
    return nodes[c] + nodes[c + 1]


GOLDEN = mtc.GOLDEN
GOLDEN_8 = os.path.join(GOLDEN, "atom_n1_8.data")
GOLDEN_216 = os.path.join(GOLDEN, "atom_n3_216.data")
