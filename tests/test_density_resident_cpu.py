"""What tests/test_gpu_density_resident.py relies on, checked where no GPU exists: the two restatements of the cells' geometry
agree by bits, the two tiers of the density reference agree on every case, the case list contains what the kernel can get
wrong, no atom sits next to a cutoff sphere; the two entries are declared and exported, the prm key defaults to false, and a
host cycle with the key set says why it does not apply."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import density_resident_reference as dr
import mesh_tables_cases as mc
import rhs_reference as rr
from gpu_util import capi, pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gmg_charge_density_resident", "gmg_get_resident_cell_geometry")
FORESTS = sorted({c[0] for c in dr.CASES})


@pytest.mark.parametrize("forest", FORESTS)
def test_geometry_restatements_agree(forest):
    """the header's formulas on the tables' vertex keys against the driver's formulas on the forest's integer coordinates"""
    s = mc.case(forest)
    a, b = dr.geometry_from_tables(s.ref, s.origin, s.h0), dr.geometry_from_forest(s.fc, s.origin, s.h0)
    for x, y, what in zip(a, b, ("cell_lo", "cell_h", "root_lo")):
        assert dr.same_bits(x, y), (forest, what)
    # the host's own tables give the same (cell_dofs and cell_level of the driver's assembly inputs)
    level, _ = dr.active_cells(s.fc)
    assert np.array_equal(level, np.asarray(s.sys.cell_level)) and len(level) == s.ref.n_cells
    # and the corners are the coordinates of the cells' first DoFs as the driver reports them
    lo = a[0]
    first = np.asarray(s.sys.cell_dofs).reshape(-1, 8)[:, 0]
    assert np.abs(lo - s.xyz[first]).max() <= 4 * np.spacing(np.abs(s.xyz).max())


@pytest.mark.parametrize("forest,n,nq,use_lists", dr.PARAMS, ids=[f"{dr.name(f, n, q)}-lists{l}" for f, n, q, l in dr.PARAMS])
def test_density_tiers_agree(forest, n, nq, use_lists):
    R = dr.reference(forest, n, nq, use_lists)
    G = R["G"]
    # a condition on the inputs, not a tolerance: no atom within 64 ulp of a cutoff sphere, so both tiers pick the same members
    assert rr.cutoff_gap_ulps(G["root_lo"], G["root_h"], G["x"], G["cutoff"]) > rr.GAP_ULPS
    rr.check_density("numpy tier", dr.name(forest, n, nq), use_lists, R, R["np"]["rho"])


def test_case_list_covers_the_kernel():
    """an empty list, lists beyond 64 and 256 atoms, three levels of cells under one root (the root, its children and
    grandchildren: a root that holds active cells of level 2 beside active cells of another level -- these forests end at
    level 2), a cell off its root's corner; and the atom counts and nq of the case table"""
    assert {c[1] for c in dr.CASES} == {0, 1, 65, 1000} and {c[2] for c in dr.CASES} == {1, 8, 27, 64, 125}
    assert {c[0] for c in dr.CASES if c[2] == 8} == {"A3", "B3", "G8-c2"} == set(FORESTS)
    longest, empty, three, off = 0, False, False, False
    for forest, n, nq in dr.CASES:
        count = dr.reference(forest, n, nq, 1)["np"]["count"]
        longest = max(longest, int(count.max()))
        empty = empty or (n > 0 and (count == 0).any() and (count > 0).any())
        G = dr.geometry(forest, n, nq)
        off = off or bool((G["cell_lo"] != G["root_lo"]).any())
        level = np.round(np.log2(G["root_h"] / G["cell_h"])).astype(int)
        roots, inv = np.unique(G["root_lo"], axis=0, return_inverse=True)
        per_root = np.zeros((len(roots), 16), bool)
        per_root[inv.reshape(-1), level] = True
        three = three or bool((per_root[:, 2:].any(1) & (per_root.sum(1) >= 2)).any())
    assert longest > 256 and empty and three and off, (longest, empty, three, off)
    counts65 = dr.reference("G8-c2", 65, 64, 1)["np"]["count"]
    assert counts65.max() <= 65 and dr.reference("A3", 1000, 8, 1)["np"]["count"].max() > 64


def test_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "gmg_coulomb.h")).read()
    declared = set(re.findall(r"\b(gmg_[a-z0-9_]+)\s*\(", text))
    L = capi().load()
    for s in NEW:
        assert s in declared and s in capi().SYMBOLS and hasattr(L, s), s
    A = capi()
    assert L.gmg_charge_density_resident(None, C.c_double(0), C.c_double(1), C.c_int64(0), None, None, C.c_double(1), C.c_double(1), C.c_int(0), C.c_int(1),
                                         None, None, None) == A.ERR_INVALID
    assert L.gmg_get_resident_cell_geometry(None, C.c_double(0), C.c_double(1), None, None, None) == A.ERR_INVALID


def test_key_defaults_to_false_and_a_host_cycle_says_why():
    S = pkg().step50
    args = dict(left=0, right=1, mesh_size=0.25, vacuum=1, problem="GaussianCharges", dim=3, bc="Homogeneous", cycles=1, r_c=0.5, global_refinement=0)
    assert "Charge densities" not in S.prm_text(**args)
    assert "set Charge densities from resident tables = true" in S.prm_text(densities_from_resident_tables=True, **args)
    golden = os.path.join(mc.GOLDEN, "atom_n1_8.data")
    p = S.Problem(S.prm_text(**args))
    p.read_lammps(golden)
    p.run_cycle(0, on_device=False)
    assert not p.densities_resident() and "Charge densities from resident tables" not in p.log()
    for more in ({}, dict(mesh_tables_on_device=True)):
        q = S.Problem(S.prm_text(densities_from_resident_tables=True, **more, **args))
        q.read_lammps(golden)
        q.run_cycle(0, on_device=False)
        assert not q.densities_resident()
        assert q.log().count("Charge densities from resident tables: not applicable (the mesh tables were not formed on the device), "
                             "per-cell arrays from the host") == 1
        assert np.array_equal(p.vector("rhs").view(np.uint64), q.vector("rhs").view(np.uint64))
        q.close()
    p.close()
