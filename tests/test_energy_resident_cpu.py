"""The CPU side of "Energy and forces from resident tables" (DESIGN.md section 25): the new symbols, the prm key and its fallback
on a host cycle, the plain-numpy node array against the host's point_locator() on every step of tests/refine_cases.py and on the
3D forests of tests/mesh_tables_cases.py, the properties of the forests that let the GPU tests catch a wrong kernel, and the
plain-Python sums against the energies a host run reports."""
import ctypes as C
import os
import re

import numpy as np

import energy_resident_cases as erc
import mesh_tables_cases as mtc
import refine_cases as rc
from gpu_util import capi, pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gmg_build_point_locator_resident", "gmg_get_point_locator", "gmg_atom_forces_resident", "gmg_electrostatic_energy_resident"]
LINE = "   Energy and forces from resident tables: not applicable ({}), host arrays"
ARGS = dict(left=0, right=1, mesh_size=0.25, vacuum=1, problem="GaussianCharges", dim=3, bc="Homogeneous", cycles=2, r_c=0.5, global_refinement=0)


def test_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "gmg_coulomb.h")).read()
    declared = set(re.findall(r"\b(gmg_[a-z0-9_]+)\s*\(", text))
    A = capi()
    L = A.load()
    for s in NEW:
        assert s in declared and s in A.SYMBOLS and hasattr(L, s), s
    for m in ("build_point_locator_resident", "get_point_locator", "atom_forces_resident", "electrostatic_energy_resident"):
        assert callable(getattr(A.Context, m)), m
    H = pkg().step50.load()
    for s in ("step50_energy_forces_resident", "step50_dof_map_builds", "step50_point_locator"):
        assert hasattr(H, s), s
    # a NULL context is refused before anything else is read
    assert L.gmg_get_point_locator(None, None, None) == A.ERR_INVALID
    assert L.gmg_build_point_locator_resident(None, C.c_int(3), None, C.c_int(0), None, None, None, None, None) == A.ERR_INVALID
    D, I = C.c_double, C.c_int64
    assert L.gmg_atom_forces_resident(None, D(0), D(1), I(0), None, None, None, I(0), D(1), D(0), None, None, None, None, None) == A.ERR_INVALID
    assert L.gmg_electrostatic_energy_resident(None, D(0), D(1), I(0), None, None, None, I(0), D(1), D(0), None, None) == A.ERR_INVALID


def host_run(**more):
    S = pkg().step50
    p = S.Problem(S.prm_text(**more, **ARGS))
    p.read_lammps(erc.GOLDEN_8)
    p.run_cycle(0, on_device=False)
    p.finish_cycle_with(np.cos(np.arange(p.n_dofs())))
    first = (p.report(-1), p.vector("solution"), p.atoms())
    p.run_cycle(1, on_device=False)
    assert not p.energy_forces_resident()
    out = (p.log(), first, p.refine_flags(), p.vector("initial_guess"), p.forest_cells())
    p.close()
    return out


def test_key_defaults_to_false_and_a_host_cycle_says_why():
    S = pkg().step50
    assert "Energy and forces from resident tables" not in S.prm_text(**ARGS)
    assert "set Energy and forces from resident tables = true" in S.prm_text(energy_forces_from_resident_tables=True, **ARGS)
    runs = [host_run(**more) for more in ({}, dict(energy_forces_from_resident_tables=True),
                                          dict(energy_forces_from_resident_tables=True, operators_from_resident_tables=True, rhs_from_cell_tables=True))]
    assert "Energy and forces from resident tables" not in runs[0][0]   # the default is false: nothing is said
    for log, first, flags, guess, fc in runs[1:]:
        assert log.count(LINE.format("Operators from resident tables did not take effect")) == 1, log   # once over two cycles
        keep = lambda text: [l for l in text.splitlines() if "not applicable" not in l and "orce" not in l]   # (other keys' lines, the forces' lines)
        assert keep(log) == keep(runs[0][0])
        for k, v in first[0].items():
            if not k.startswith("force") and not k.endswith("seconds") and not k.endswith("_ms"):
                assert repr(v) == repr(runs[0][1][0][k]), k
        assert np.array_equal(rc.bits(first[1]), rc.bits(runs[0][1][1])) and np.array_equal(flags, runs[0][2])
        assert np.array_equal(rc.bits(guess), rc.bits(runs[0][3]))
        rc.same_forest(fc, runs[0][4])


def test_node_array_on_every_step():
    """the restatement reproduces the host's point_locator() on the forest that goes into every step and on the one it leaves"""
    n = 0
    for name in rc.STEPS:
        s = rc.step(name)
        fc, node, new_fc, new_node = erc.host_nodes(name)
        rc.same_forest(fc, s.fc, name)
        rc.same_forest(new_fc, s.new_fc, name)
        for f, want in ((s.fc, node), (s.new_fc, new_node)):
            got = erc.node_array(f)
            assert got.dtype == want.dtype and np.array_equal(got, want), name
            assert (got < 0).sum() == (np.asarray(f.cell_first_child).reshape(-1) < 0).sum()
        n += 1
    assert n == len(rc.STEPS) >= 10


def test_node_array_on_the_3d_forests_of_the_mesh_table_cases():
    """the same for the 3D forests of tests/mesh_tables_cases.py: cell number -node - 1 of an active cell is the row of the
    tables' cell_dofs (first-touch restatement of tests/mesh_tables_reference.py), and the families' forests are those the
    host's array was checked on above"""
    seen = 0
    for name, (family, cycle) in mtc.CASES.items():
        snap = mtc.case(name)
        if snap.fc.dim != 3:
            continue
        node = erc.node_array(snap.fc)
        active = np.flatnonzero(node < 0)
        assert np.array_equal(-node[active] - 1, np.arange(snap.ref.n_cells)), name
        if family in rc.FAMILIES and cycle <= rc.FAMILIES[family]:
            steps = [n for n in rc.STEPS if n.split(":")[0] == family]
            fc, host = erc.host_nodes(steps[min(cycle, len(steps) - 1)])[0:2] if cycle < len(steps) else erc.host_nodes(steps[-1])[2:4]
            rc.same_forest(fc, snap.fc, name)
            assert np.array_equal(node, host), name
            seen += 1
    assert seen >= 4


def test_the_cases_can_catch_a_wrong_kernel():
    root_active = deep = between = False
    for name in erc.FORESTS:
        fc = erc.forest(name)
        assert fc.dim == 3 and fc.level0_lexicographic
        a, d, b = erc.properties(fc)
        root_active |= a
        deep |= d
        between |= b
    assert root_active and deep and between
    assert erc.properties(erc.forest("deep")) == (True, True, True)
    sizes = [len(np.asarray(erc.forest(n).cell_first_child).reshape(-1)) for n in erc.FORESTS]
    assert min(sizes) == 8 and 200 <= max(sizes) <= 450, sizes
    a = d = b = False
    for name in rc.STEPS:
        pa, pd, pb = erc.properties(rc.step(name).new_fc)
        a, d, b = a | pa, d | pd, b | pb
    assert a and b   # (the driven steps stay shallower than three levels: "deep" is the hand-built forest's)
    # the atom sets: 40 distinct atoms, some outside the box on every side
    for gname, (origin, h0) in erc.GEOMETRY.items():
        for name in erc.FORESTS:
            fc = erc.forest(name)
            xyz, q = erc.atom_set(fc, origin, h0, 40)
            t = (xyz - origin) / h0
            assert xyz.shape == (40, 3) and len(q) == 40 and (t < 0).any() and (t > np.array(fc.n0)).any(), (gname, name)
            assert erc.atom_set(fc, origin, h0, 1)[0].shape == (1, 3) and erc.atom_set(fc, origin, h0, 0)[0].shape == (0, 3)
    # exactly on: with the binary pair the lattice coordinate of the interface points is recovered without rounding
    origin, h0 = erc.GEOMETRY["binary"]
    xyz, _ = erc.atom_set(erc.forest("deep"), origin, h0, 40)
    t = (xyz - origin) / h0
    assert t[0, 0] == 1.0 and tuple(t[2, :2]) == (1.0, 1.0) and tuple(t[6]) == (0.75, 0.75, 0.75) and tuple(t[8]) == (0.875, 0.875, 0.875)


def test_the_sums_are_the_host_s():
    """fe_long and self of a host run are the plain-Python sums of q and the host's phi_h at the atoms, by bits"""
    S = pkg().step50
    for cutoff in (0.0, 2.5):
        p = S.Problem(S.prm_text(short_range_cutoff=cutoff, **ARGS))
        p.read_lammps(erc.GOLDEN_8)
        p.run_cycle(0, on_device=False)
        p.finish_cycle_with(np.cos(np.arange(p.n_dofs())))
        rep = p.report(-1)
        q, xyz = p.atoms()
        phi, _, _, _, e_short = p.atom_forces(on_device=False, cutoff=cutoff, parts=True)
        p.close()
        short, fe, self_e = erc.energy_sums(q, phi, e_short, 0.5)
        assert np.float64(fe).tobytes() == np.float64(rep["energy_fe_long"]).tobytes(), (fe, rep["energy_fe_long"])
        assert np.float64(self_e).tobytes() == np.float64(rep["energy_self"]).tobytes(), (self_e, rep["energy_self"])
        xyz = np.asarray(xyz, float).reshape(-1, 3)
        ref = erc.ar.pair_sums_numpy(xyz, np.asarray(q, float), 0.5, cutoff)
        bound = erc.short_bound(ref) + erc.host_short_bound(xyz, np.asarray(q, float), 0.5, cutoff, ref)
        print(f"cutoff {cutoff}: host short {rep['energy_short']!r}, sum of the mirror's e_short {short!r}, bound {bound:.3e}")
        assert abs(short - rep["energy_short"]) <= bound and abs(short - ref["e"].sum()) <= erc.short_bound(ref)
