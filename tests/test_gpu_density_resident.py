"""gmg_charge_density_resident and gmg_get_resident_cell_geometry on the MI355X (csrc/gmg_density.hpp)
through the C ABI: the geometry by bits against the restatements of tests/density_resident_reference.py; the densities against
both tiers of tests/rhs_reference.py and against the sibling gmg_charge_density fed the downloaded geometry; the same bits for
every launch shape; the special values; the copy that stays on the device and what consumes it; the refusals; the device
memory over six rounds; and whole runs of the driver with "Charge densities from resident tables" off and on."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import atoms_reference as ar
import density_resident_reference as dr
import mesh_tables_cases as mc
import rhs_reference as rr
from gpu_util import capi, pkg
from test_rhs_reference_cpu import E2E_CUT, E2E_RC, end_to_end_problem

pytestmark = pytest.mark.gpu
IDS = [f"{dr.name(f, n, q)}-lists{l}" for f, n, q, l in dr.PARAMS]


def build(c, fc):
    return c.build_mesh_tables(dim=fc.dim, n0=fc.n0, n_levels=fc.n_levels, level_ptr=fc.level_ptr, cell_coord=fc.cell_coord,
                               cell_first_child=fc.cell_first_child, level0_lexicographic=fc.level0_lexicographic)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def refused(code, call, text=None):
    with pytest.raises(capi().GMGError) as e:
        call()
    assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)
    return True


def resident(c, G, use_lists, dens=True, **kw):
    return c.charge_density_resident(G["origin"], G["h0"], G["x"], G["q"], G["r_c"], G["cutoff"], use_lists, G["qp"], dens=dens, **kw)[0]


def no_densities(c, n_cells, nq):
    return refused(capi().ERR_INVALID, lambda: c.get_charge_density(n_cells, nq), "no densities")


@pytest.fixture(scope="module")
def contexts():
    """one context per forest, its tables built once"""
    made = {}

    def get(forest):
        if forest not in made:
            made[forest] = capi().Context(1)
            build(made[forest], mc.case(forest).fc)
        return made[forest]

    yield get
    for c in made.values():
        c.close()


# ------------------------------------------------------------------------------------------------ 1. geometry

@pytest.mark.parametrize("forest", sorted({c[0] for c in dr.CASES}))
def test_geometry_by_bits(contexts, forest):
    s = mc.case(forest)
    c = contexts(forest)
    for max_blocks in (0, 1, 3):
        c.set_option("assemble_max_blocks", max_blocks)
        got = c.get_resident_cell_geometry(s.origin, s.h0)
        for ref in (dr.geometry_from_tables(c.get_mesh_tables(), s.origin, s.h0), dr.geometry_from_tables(s.ref, s.origin, s.h0),
                    dr.geometry_from_forest(s.fc, s.origin, s.h0)):   # the device's own tables, their restatement, the host's arrays
            for a, b, what in zip(got, ref, ("cell_lo", "cell_h", "root_lo")):
                assert dr.same_bits(a, b), (forest, max_blocks, what)
    c.set_option("assemble_max_blocks", 0)
    lo, hh, rlo = c.get_resident_cell_geometry(s.origin, s.h0, want=(False, True, False))   # NULL arrays are skipped
    assert lo is None and rlo is None and dr.same_bits(hh, got[1])
    # another origin and root edge: nothing is cached
    other = c.get_resident_cell_geometry(-0.3, 0.7)
    for a, b in zip(other, dr.geometry_from_forest(s.fc, -0.3, 0.7)):
        assert dr.same_bits(a, b)


# ------------------------------------------------------------------------------------------------ 2. densities

@pytest.mark.parametrize("forest,n,nq,use_lists", dr.PARAMS, ids=IDS)
def test_densities_against_the_references_and_the_sibling(contexts, forest, n, nq, use_lists):
    R = dr.reference(forest, n, nq, use_lists)
    G = R["G"]
    c = contexts(forest)
    rho = resident(c, G, use_lists)
    rr.check_density("resident", dr.name(forest, n, nq), use_lists, R, rho)   # mpmath: the bound; numpy: twice the bound; +0.0 for empty lists
    assert no_densities(c, *rho.shape)   # a host array keeps none on the device
    # the sibling in a second context, fed the geometry this entry works with
    lo, hh, rlo = c.get_resident_cell_geometry(G["origin"], G["h0"])
    b = capi().Context(1)
    sib = b.charge_density(lo, hh, rlo, G["h0"], G["x"], G["q"], G["r_c"], G["cutoff"], use_lists, G["qp"])
    b.close()
    r = rr.ratio(rho - sib, 2.0 * R["np"]["bound"])
    print(f"resident vs sibling {dr.name(forest, n, nq)} lists {use_lists}: difference / (2 x numpy bound) {r:.2e}")
    assert r <= 1.0
    assert np.array_equal(rho == 0.0, sib == 0.0)
    # kept on the device: the same bits come back, in the sibling's place
    assert resident(c, G, use_lists, dens=None) is None
    assert np.array_equal(bits(c.get_charge_density(*rho.shape)), bits(rho))
    assert refused(capi().ERR_INVALID, lambda: c.get_charge_density(rho.shape[0] + 1, nq))


@pytest.mark.parametrize("forest,n,nq,use_lists", dr.PARAMS, ids=IDS)
def test_bits_do_not_depend_on_the_launch_shape(contexts, forest, n, nq, use_lists):
    G = dr.geometry(forest, n, nq)
    c = contexts(forest)
    first = resident(c, G, use_lists)
    assert np.array_equal(bits(resident(c, G, use_lists)), bits(first))   # two calls in a row
    for max_blocks, segment in ((1, 0), (3, 0), (0, 1), (3, 9), (0, 2047)):   # one workgroup; three; the shortest, a short and the longest segment
        c.set_option("assemble_max_blocks", max_blocks)
        c.set_option("density_segment", segment)
        assert np.array_equal(bits(resident(c, G, use_lists)), bits(first)), (max_blocks, segment)
    c.set_option("assemble_max_blocks", 0)
    c.set_option("density_segment", 0)


def test_special_values(contexts):
    """+0.0 with an unset sign: empty lists among full ones, zero atoms with and without lists, a cutoff of 0"""
    for forest, n, nq in (("A3", 1000, 8), ("A3", 0, 1), ("G8-c2", 65, 64)):
        G = dr.geometry(forest, n, nq)
        c = contexts(forest)
        count = dr.reference(forest, n, nq, 1)["np"]["count"]
        rho = resident(c, G, 1)
        assert (count == 0).any() and np.all(bits(rho[count == 0]) == 0), (forest, n)
        assert np.all(rho[count > 0] != 0.0)
        if n == 0:
            assert np.all(bits(resident(c, G, 0)) == 0)
    G = dict(dr.geometry("A3", 65, 125), cutoff=0.0)
    assert np.all(bits(resident(contexts("A3"), dict(G, x=G["x"][:1], q=G["q"][:1]), 1)) == 0)   # nobody is closer than 0 (one atom: one bin)


# ------------------------------------------------------------------------------------------------ 3. what consumes them

@functools.lru_cache(maxsize=None)
def lattice_case(use_lists):
    """cycle 0 of the driver on the host for the gas of tests/test_rhs_reference_cpu.py: the forest, the inputs of the right-hand
    side, the DoF coordinates, and the right-hand side built from them alone with its bound"""
    p, x, q = end_to_end_problem(use_lists)
    p.run_cycle(0, on_device=False)
    fc, inp, X, free = p.forest_cells(), p.rhs_assembly_inputs(), p.dof_coordinates(), ~p.constrained_mask()
    p.close()
    ref, bound, gap = rr.end_to_end_reference(X, x, q, E2E_RC, E2E_CUT * E2E_RC, 2, use_lists)
    assert gap > 1e-9
    origin, h0 = mc._lattice_geometry(0.0, 1.0, 0.25, 10)   # (the prm of end_to_end_problem)
    assert origin == X.min() and origin + h0 == np.unique(X[:, 0])[1]
    return dict(fc=fc, inp=inp, free=free, ref=ref, bound=bound, x=x, q=q, origin=float(origin), h0=float(h0))


@pytest.mark.parametrize("use_lists", [False, True])
def test_right_hand_side_from_the_resident_densities(use_lists):
    """gmg_assemble_rhs_resident(source = NULL) on the densities this entry left, against the same call on densities the sibling
    left and against the right-hand side built from the DoF coordinates alone"""
    A = capi()
    T = lattice_case(use_lists)
    qp = ar.gauss_rule(2)[0]
    n = T["inp"].n_dofs
    out = []
    for which in ("resident", "sibling"):
        c = A.Context(1)
        build(c, T["fc"])
        c.close_constraints(None)   # homogeneous boundary values
        if which == "resident":
            c.charge_density_resident(T["origin"], T["h0"], T["x"], T["q"], E2E_RC, E2E_CUT * E2E_RC, use_lists, qp, dens=None)
        else:
            lo, hh, rlo = c.get_resident_cell_geometry(T["origin"], T["h0"])
            c.charge_density(lo, hh, rlo, T["h0"], T["x"], T["q"], E2E_RC, E2E_CUT * E2E_RC, use_lists, qp, dens=None)
        v = c.vector(n, np.full(n, 7.0))
        c.assemble_rhs_resident(T["inp"], v, source=None)
        out.append(v.download())
        c.close()
    free, bound = T["free"], T["bound"]
    r_sib = rr.ratio((out[0] - out[1])[free], bound[free])
    r_ref = max(rr.ratio((o - T["ref"])[free], 2.0 * bound[free]) for o in out)
    print(f"rhs from resident densities, lists {int(use_lists)}: vs sibling / bound {r_sib:.2e}, vs the reference / (2 x bound) {r_ref:.2e}")
    assert (T["ref"][free] != 0).sum() > 500 and r_sib <= 1.0 and r_ref <= 1.0


def test_estimator_takes_the_resident_densities(contexts):
    """gmg_estimate_error(residual, dens = NULL) finds what this entry left: the residual term equals the one from the same
    densities passed as a host array"""
    S = pkg().step50
    p = S.Problem(S.prm_text(left=0, right=1, mesh_size=0.25, vacuum=1, problem="GaussianCharges", dim=3, bc="Homogeneous", cycles=2, r_c=0.5, cutoff=3.5,
                             rhs_optimization=True, quad_rhs=1, global_refinement=0))
    p.read_lammps(os.path.join(mc.GOLDEN, "atom_n1_8.data"))
    p.run_cycle(0, on_device=False)
    e, fc, X = p.estimator_inputs(), p.forest_cells(), p.dof_coordinates()
    p.close()
    origin, h0 = mc._lattice_geometry(0.0, 1.0, 0.25, 1)
    assert origin == X.min() and origin + h0 == np.unique(X[:, 0])[1]
    x, q, _ = ar.gas(31, 8, 0.5)
    c = capi().Context(1)
    build(c, fc)
    qp = ar.gauss_rule(round(len(e.weight) ** (1.0 / 3.0)))[0]
    assert len(qp) == len(e.weight)
    args = (origin, h0, x - ar.LO, q, 0.5, 1.75, True, qp)
    rho, _ = c.charge_density_resident(*args)
    u = c.vector(e.n_u, np.cos(np.arange(e.n_u, dtype=np.float64)))

    def estimate(dens):
        return c.estimate_error(e.dim, e.cell_dofs, e.cell_level, e.face_kind, e.face_cell, e.h_of_level, e.face_measure_of_level, e.diameter_of_level,
                                e.gauss_x, e.gauss_w, u, 2, e.weight, e.jxw_of_level, dens, e.fraction)

    assert refused(capi().ERR_INVALID, lambda: estimate(None), "densities")   # the host-array call left none
    c.charge_density_resident(*args, dens=None)
    a, b = estimate(None), estimate(rho)
    assert np.array_equal(bits(a.residual_sq), bits(b.residual_sq)) and (a.residual_sq != 0).any()
    c.close()


# ------------------------------------------------------------------------------------------------ 4. refusals, memory

def test_refusals_and_no_densities_afterwards():
    A = capi()
    forest, n, nq = "B3", 65, 8
    G = dr.geometry(forest, n, nq)
    s = mc.case(forest)
    nc = len(G["cell_h"])
    c = A.Context(1)
    assert refused(A.ERR_INVALID, lambda: resident(c, G, 1, n_cells=nc), "no mesh tables")
    assert refused(A.ERR_INVALID, lambda: c.get_resident_cell_geometry(G["origin"], G["h0"]), "no mesh tables")
    build(c, s.fc)

    def after(code, text, **change):
        """with densities on the device, the call is refused and they are gone"""
        assert resident(c, G, 1, dens=None) is None and c.get_charge_density(nc, nq).shape == (nc, nq)
        H = dict(G, **{k: v for k, v in change.items() if k in G})
        kw = {k: v for k, v in change.items() if k not in G}
        for dens in (True, None):
            assert refused(code, lambda: resident(c, H, 1, dens=dens, **kw), text), change.keys()
            assert no_densities(c, nc, nq)

    after(A.ERR_INVALID, "nq", qp=np.zeros((0, 3)))
    after(A.ERR_INVALID, "r_c", r_c=0.0)
    after(A.ERR_INVALID, "r_c", r_c=-0.5)
    after(A.ERR_INVALID, "r_c", r_c=float("nan"))
    after(A.ERR_INVALID, "h0", h0=0.0)
    after(A.ERR_INVALID, "h0", h0=-1.0)
    after(A.ERR_INVALID, "cutoff", cutoff=-1e-300)
    after(A.ERR_INVALID, "NULL", x=None, n_atoms=n)
    after(A.ERR_INVALID, "NULL", q=None, n_atoms=n)
    after(A.ERR_INVALID, "NULL", qp=None, nq=nq)
    after(A.ERR_INVALID, "n_atoms", n_atoms=-1)
    far = G["x"].copy()
    far[0] += 1e9 * G["cutoff"]
    after(A.ERR_UNSUPPORTED, "bin grid", x=far)   # the sibling's case: more than 2^28 bins
    assert refused(A.ERR_INVALID, lambda: c.get_resident_cell_geometry(G["origin"], 0.0), "h0")
    # valid: zero atoms, NULL atoms of zero length; then zero cells
    assert np.all(bits(resident(c, dict(G, x=None, q=None), 1)) == 0)
    import mesh_tables_reference as mtr
    build(c, mtr.empty(3))
    assert resident(c, G, 1, n_cells=0).shape == (0, nq) and resident(c, G, 1, dens=None) is None
    assert [a.shape for a in c.get_resident_cell_geometry(0.0, 1.0)] == [(0, 3), (0,), (0, 3)]
    # 2D tables
    build(c, mtr.quadrant_2d())
    assert refused(A.ERR_UNSUPPORTED, lambda: resident(c, G, 1, n_cells=4), "3D")
    assert refused(A.ERR_UNSUPPORTED, lambda: c.get_resident_cell_geometry(0.0, 1.0), "3D")
    # after gmg_reset the tables are gone; the context still works
    build(c, s.fc)
    assert c.L.gmg_reset(c.h, C.c_int(1)) == A.OK
    assert refused(A.ERR_INVALID, lambda: resident(c, G, 1, n_cells=nc), "no mesh tables")
    build(c, s.fc)
    assert np.array_equal(bits(resident(c, G, 1)), bits(resident(c, G, 1)))
    c.close()


def test_unsupported_on_a_communicator():
    A = capi()
    G = dr.geometry("B3", 65, 8)
    c = A.Context(1)
    c.comm_init(0, 1, A.Context.unique_id())
    assert refused(A.ERR_UNSUPPORTED, lambda: resident(c, G, 1, n_cells=len(G["cell_h"])), "communicator")
    assert refused(A.ERR_UNSUPPORTED, lambda: c.get_resident_cell_geometry(G["origin"], G["h0"]), "communicator")
    c.close()


def test_no_leak_over_six_rounds():
    """as tests/test_gpu_lifecycle.py: build, densities (copied out and kept), geometry, reset, six times in one context; the free
    device memory after the last round equals that after the first"""
    import torch

    G = dr.geometry("B3", 65, 8)
    s = mc.case("B3")
    c = capi().Context(1)
    free = []
    for _ in range(6):
        build(c, s.fc)
        assert resident(c, G, 1).shape == (len(G["cell_h"]), 8)
        assert resident(c, G, 0, dens=None) is None
        assert c.get_resident_cell_geometry(G["origin"], G["h0"])[1].shape == (len(G["cell_h"]),)
        assert refused(capi().ERR_INVALID, lambda: resident(c, dict(G, r_c=0.0), 1))   # (drops what the call before kept)
        assert resident(c, G, 1, dens=None) is None
        assert c.L.gmg_reset(c.h, C.c_int(1)) == capi().OK
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    c.close()
    print("free device memory after each round, relative to the first:", [f - free[0] for f in free])
    assert free[-1] == free[0], free


# ------------------------------------------------------------------------------------------------ 5. whole runs of the driver

ALL_KEYS = dict(mesh_tables_on_device=True, system_matrix_on_device=True, level_matrices_on_device=True, rhs_from_cell_tables=True,
                operators_from_resident_tables=True, estimator_on_device=True, analytical_on_device=True, refinement_on_device=True, transfer_on_device=True)
LINE = "Charge densities from resident tables: not applicable ({}), per-cell arrays from the host"


def golden_problem(name, right, cycles, vacuum, key, **more):
    S = pkg().step50
    args = dict(ALL_KEYS)
    args.update(more)
    p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=vacuum, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=cycles, r_c=0.5,
                             cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR", densities_from_resident_tables=key, **args))
    p.read_lammps(os.path.join(mc.GOLDEN, name))
    return p


def read_atoms(name):
    """charges and positions of a golden LAMMPS file (atom style full): lines `id molecule type q x y z` after `Atoms`"""
    q, x = [], []
    seen = False
    for line in open(os.path.join(mc.GOLDEN, name)):
        f = line.split()
        if f[:1] == ["Atoms"]:
            seen = True
        elif seen and len(f) >= 7:
            q.append(float(f[3])); x.append([float(v) for v in f[4:7]])
    return np.array(q), np.array(x)


@pytest.mark.parametrize("name,right,cycles,vacuum,estimator", [("atom_n1_8.data", 1.0, 3, 10, "Kelly + residual"), ("atom_n3_216.data", 3.0, 2, 2, "Kelly")],
                         ids=["8-atoms-3-cycles", "216-atoms-2-cycles"])
def test_driver_runs_with_the_key_off_and_on(name, right, cycles, vacuum, estimator, monkeypatch):
    """every other `... on device` key set, the driver holding the device's geometry against its own loop in every cycle
    (STEP50_CHECK_RESIDENT): equal cell and DoF counts, refinement marks, outer and coarse iteration counts in every cycle; on
    the full lattice of cycle 0, where tests/rhs_reference.py builds the right-hand side from the DoF coordinates alone, both
    runs' system_rhs within twice its bound of that reference and within twice the bound of each other"""
    monkeypatch.setenv("STEP50_CHECK_RESIDENT", "1")
    runs = {}
    for key in (False, True):
        p = golden_problem(name, right, cycles, vacuum, key, refinement_estimator=estimator)
        out = []
        for cycle in range(cycles):
            rep = p.run_cycle(cycle, on_device=True)
            assert p.densities_resident() == key and p.mesh_tables_on_device() and p.operators_resident(), (key, cycle)
            out.append((rep, p.refine_flags(), p.vector("rhs"), p.dof_coordinates() if cycle == 0 else None, ~p.constrained_mask()))
        assert "Charge densities from resident tables" not in p.log(), p.log()   # no fallback line
        runs[key] = out
        p.close()
    q, x = read_atoms(name)
    for cycle, (a, b) in enumerate(zip(runs[False], runs[True])):
        for k in ("active_cells", "dofs", "dofs_by_level", "cg_iterations", "coarse_iterations", "n_levels", "status"):
            assert a[0][k] == b[0][k], (cycle, k, a[0][k], b[0][k])
        assert np.array_equal(a[1], b[1]), cycle
        assert a[2].shape == b[2].shape
    a, b = runs[False][0], runs[True][0]
    # (the golden atoms and the lattice are multiples of 1 / 8, the cutoff is 1.75: every distance of the list predicate is
    # formed exactly, so an atom ON a cutoff sphere -- there are some -- is off the list for the host, the device and the reference)
    assert np.all(x * 8 == np.round(x * 8)) and np.all(a[3] * 8 == np.round(a[3] * 8))
    ref, bound, _ = rr.end_to_end_reference(a[3], x, q, 0.5, 1.75, 2, True)
    free = a[4]
    r_ref = max(rr.ratio((v[2] - ref)[free], 2.0 * bound[free]) for v in (a, b))
    r_each = rr.ratio((a[2] - b[2])[free], 2.0 * bound[free])
    print(f"driver {name}: system_rhs of cycle 0, key on vs off / (2 x bound) {r_each:.2e}, vs the reference / (2 x bound) {r_ref:.2e}")
    assert (ref[free] != 0).sum() > 100 and r_ref <= 1.0 and r_each <= 1.0
    assert runs[True][-1][0]["cg_iterations"] >= 1 and len(runs[True][-1][0]["dofs_by_level"]) >= 2


@pytest.mark.parametrize("missing,why", [("mesh_tables_on_device", "the mesh tables were not formed on the device"),
                                         ("densities_on_device", "Charge densities on device is not set")])
def test_a_missing_prerequisite_keeps_the_host_arrays(missing, why):
    """one line says why, once over two cycles, and the run is the one without the key"""
    more = {missing: False}
    if missing == "mesh_tables_on_device":
        more["operators_from_resident_tables"] = False   # (it needs the tables too and would say so itself)
    p, q = (golden_problem("atom_n1_8.data", 1.0, 2, 2, key, refinement_estimator="Kelly", **more) for key in (True, False))
    for cycle in range(2):
        r1, r0 = p.run_cycle(cycle, on_device=True), q.run_cycle(cycle, on_device=True)
        assert not p.densities_resident() and r1["cg_iterations"] == r0["cg_iterations"]
        assert np.array_equal(bits(p.vector("rhs")), bits(q.vector("rhs"))) and np.array_equal(bits(p.vector("solution")), bits(q.vector("solution")))
    assert p.log().count(LINE.format(why)) == 1 and "Charge densities from resident tables" not in q.log()
    p.close()
    q.close()


def test_other_problems_keep_the_host_path():
    """a distributed run, a problem without LAMMPS input and a 2D one: one line each, the run goes on"""
    from test_coef_matrix_cpu import step16_problem

    p = golden_problem("atom_n1_8.data", 1.0, 1, 2, True, refinement_estimator="Kelly")
    p.set_communicator(0, 1, capi().Context.unique_id())
    p.run_cycle(0, on_device=True)
    assert not p.densities_resident() and p.log().count(LINE.format("the run is distributed")) == 1
    p.close()
    for dim, why in ((3, "no LAMMPS input"), (2, "the problem is not 3D")):
        p = step16_problem(dim, 2, 2, mesh_tables_on_device=True, densities_from_resident_tables=True)
        for cycle in range(2):
            p.run_cycle(cycle, on_device=True)
        assert not p.densities_resident() and p.log().count(LINE.format(why)) == 1
        p.close()
