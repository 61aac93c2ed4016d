"""Option ssor_plan_device on the MI355X (csrc/gmg_sgs_plan.hpp): the SSOR plan of a level formed by
kernels against the host builder's plan of a second context with the option off -- all ten plan arrays byte for byte, the
plan's numbers, the partition and the backward rows, then (and only then: a wrong plan fails here before it reaches the
sweep kernel) one smoother step from zero and one from a start vector, bit for bit.  The cases and what is expected of each
are in tests/ssor_plan_cases.py; no case can pass by quietly falling back."""
import ctypes as C

import numpy as np
import pytest

import ssor_plan_cases as spc
from gpu_util import capi
from test_gpu_level_matrices import assemble

pytestmark = pytest.mark.gpu
LEVEL = 1


def context(m, blocks, options=(), bounds=False, device=False, max_blocks=0, upload=True):
    A = capi()
    c = A.Context(2)
    c.set_tuning(ssor_blocks=blocks)
    for key, value in options:
        c.set_option(key, value)
    if device:
        c.set_option("ssor_plan_device", 1)
        c.set_option("assemble_max_blocks", max_blocks)
    if bounds:
        c.set_ssor_block_rows(LEVEL, spc.given_bounds(m.n_rows))
    c.set_smoother(A.SSOR, 0.5, 2)
    if upload:
        c.set_level_matrix(LEVEL, m)
    return c


def plan_of(c, level=LEVEL):
    """everything the accessors tell about a level's plan; arrays: None for a level without a four-wave plan"""
    A = capi()
    try:
        arrays = {w: c.get_ssor_plan_array(level, w).tobytes() for w in A.SSOR_PLAN_ARRAYS}
    except A.GMGError as e:
        assert e.code == A.ERR_INVALID
        arrays = None
    br, steps = c.get_ssor_partition(level)
    return dict(arrays=arrays, plan=c.get_ssor_plan(level), block_row=br.tolist(), block_steps=steps.tolist(), bwd=c.get_ssor_backward_rows(level).tolist())


def assert_same_plan(dev, host, what):
    if host["arrays"] is None:
        assert dev["arrays"] is None, what
    else:
        for w, ref in host["arrays"].items():
            assert dev["arrays"][w] == ref, (what, w, len(ref))
    for k in ("plan", "block_row", "block_steps", "bwd"):
        assert dev[k] == host[k], (what, k)


def steps(c, n, level=LEVEL):
    rng = np.random.default_rng(n)
    u0, rhs = rng.standard_normal(n), rng.standard_normal(n)
    out = []
    for from_zero in (True, False):
        u, r = c.vector(n, u0), c.vector(n, rhs)
        c.smoother_step(level, u, r, from_zero)
        out.append(u.download().view(np.uint64))
    return out


def compare(case, blocks, max_blocks_list):
    m = case.make()
    host = context(m, blocks, case.options, case.bounds)
    assert host.get_ssor_plan_origin(LEVEL) == (False, 0, "")
    ref_plan, ref_steps = plan_of(host), steps(host, m.n_rows)
    host.close()
    for mb in max_blocks_list:
        dev = context(m, blocks, case.options, case.bounds, device=True, max_blocks=mb)
        on_device, moved, why = dev.get_ssor_plan_origin(LEVEL)
        assert (spc.DEVICE if on_device else why) == case.expect, (case.name, blocks, mb, on_device, why)
        assert moved == 0
        assert_same_plan(plan_of(dev), ref_plan, (case.name, blocks, mb))
        got = steps(dev, m.n_rows)   # (only after the plans compared equal)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref_steps)), (case.name, blocks, mb)
        dev.close()
    return ref_plan, ref_steps


@pytest.mark.parametrize("run", spc.runs(spc.DEVICE_CASES), ids=spc.run_id)
def test_device_plan_is_the_host_plan(run):
    case, blocks = run
    ref_plan, _ = compare(case, blocks, spc.MAX_BLOCKS)
    assert ref_plan["arrays"] is not None   # (the host plan is a four-wave plan: the comparison above compared arrays)


@pytest.mark.parametrize("run", spc.runs(spc.FALLBACK_CASES), ids=spc.run_id)
def test_fallback_reports_its_reason_and_carries_the_host_plan(run):
    case, blocks = run
    compare(case, blocks, spc.MAX_BLOCKS)


def test_one_rank_communicator_keeps_the_host_plan():
    """a context on a communicator (one rank, formed as tests/test_gpu_resident.py forms it; one context, since forming a
    communicator takes seconds): with the option the host plans as without it, and says why"""
    A = capi()
    m = spc.lattice27(9)
    c = A.Context(2)
    c.comm_init(0, 1, A.Context.unique_id())
    c.set_tuning(ssor_blocks=3)
    c.set_smoother(A.SSOR, 0.5, 2)
    out = []
    for device in (False, True):
        c.set_option("ssor_plan_device", int(device))
        c.set_level_matrix(LEVEL, m)
        assert c.get_ssor_plan_origin(LEVEL) == (False, 0, "communicator" if device else "")
        out.append((plan_of(c), steps(c, m.n_rows)))
    assert out[0][0]["arrays"] is not None
    assert_same_plan(out[1][0], out[0][0], "communicator")
    assert all(np.array_equal(a, b) for a, b in zip(out[1][1], out[0][1]))
    c.close()


RESIDENT_FORMS = [("A3", False), ("B3", False), ("S2-c2", False), ("S2-c2", True)]


@pytest.mark.parametrize("name,coef", RESIDENT_FORMS, ids=[f"{n}{'-coef' if k else ''}" for n, k in RESIDENT_FORMS])
def test_resident_form_downloads_no_csr(name, coef):
    """gmg_assemble_level_matrix_resident (and its _coef sibling on the 2D Step16 case) on the context's own mesh tables, with
    the option against without it: the ten arrays and the plan's numbers first, then the origin, the steps last"""
    import resident_cases as rc
    from test_gpu_resident import load_level, resident_context

    A = capi()
    x = rc.case(name)
    L = len(x.levels)
    for blocks, mb in ((1, 0), (3, 1), (3, 3)):
        a, b = resident_context(x, L), resident_context(x, L)
        for c in (a, b):
            c.set_tuning(ssor_blocks=blocks)
            c.set_smoother(A.SSOR, 0.5, 2)
            c.set_option("assemble_max_blocks", mb)
        a.set_option("ssor_plan_device", 1)
        for l in range(L):
            load_level(a, x, l, True, coef)
            load_level(b, x, l, True, coef)
            if l == 0:
                continue
            assert_same_plan(plan_of(a, l), plan_of(b, l), (name, coef, l, blocks, mb))
            assert a.get_ssor_plan_origin(l) == (True, 0, "")
            on_device, moved, why = b.get_ssor_plan_origin(l)
            assert (on_device, why) == (False, "") and moved > 0
            n = x.levels[l].n_dofs
            assert all(np.array_equal(u, v) for u, v in zip(steps(a, n, l), steps(b, n, l))), (name, coef, l, blocks, mb)
        a.close()
        b.close()


@pytest.mark.parametrize("name,level", [("A3", 1), ("A3", 2), ("B3", 1), ("B3", 2)])
def test_adaptive_levels_also_equal_the_oracle(name, level):
    """as tests/test_gpu_ssor_sliding.py: the step of a device-planned level against OracleMG.smooth, bit for bit"""
    import mg_cases
    from oracle import gmg_oracle as go

    h = mg_cases.hierarchy(name)[0]
    m = h.level_matrices[level]
    n = m.n_rows
    for blocks in (1, 3):
        host, dev = context(m, blocks), context(m, blocks, device=True)
        assert dev.get_ssor_plan_origin(LEVEL)[0] and not host.get_ssor_plan_origin(LEVEL)[0]
        assert_same_plan(plan_of(dev), plan_of(host), (name, level, blocks))
        mg = go.OracleMG(h, smoother=go.SSOR, ssor_blocks=blocks)
        rng = np.random.default_rng(n)
        u0, rhs = rng.standard_normal(n), rng.standard_normal(n)
        for k, from_zero in enumerate((True, False)):
            ref = mg.smooth(level, u0, rhs, from_zero).view(np.uint64)
            assert np.array_equal(steps(dev, n)[k], ref) and np.array_equal(steps(host, n)[k], ref), (name, level, blocks, from_zero)
        host.close()
        dev.close()


@pytest.mark.parametrize("name", ("A3", "B3", "2D"))
def test_assembled_levels_download_no_csr(name):
    """gmg_assemble_level_matrix with the option: the same plans as without it, and no byte of col / val comes back"""
    from test_level_matrix_cpu import case

    A = capi()
    levels = case(name).levels
    for blocks, mb in ((1, 0), (3, 1), (3, 3)):
        a, b = A.Context(len(levels)), A.Context(len(levels))
        for c in (a, b):
            c.set_tuning(ssor_blocks=blocks)
            c.set_smoother(A.SSOR, 0.5, 2)
        a.set_option("ssor_plan_device", 1)
        a.set_option("assemble_max_blocks", mb)
        b.set_option("assemble_max_blocks", mb)
        for l, x in enumerate(levels):
            assemble(a, l, x.inp)
            assemble(b, l, x.inp)
            if l == 0:
                continue
            assert a.get_ssor_plan_origin(l) == (True, 0, "")
            assert b.get_ssor_plan_origin(l) == (False, 12 * x.host_A.nnz, "")
            assert_same_plan(plan_of(a, l), plan_of(b, l), (name, l, blocks, mb))
            n = x.inp.n_dofs
            assert all(np.array_equal(u, v) for u, v in zip(steps(a, n, l), steps(b, n, l))), (name, l, blocks, mb)
        a.close()
        b.close()


def test_switching_the_option_with_a_reupload_and_reset():
    A = capi()
    m = spc.lattice27(9)
    host = context(m, 3)
    ref_plan, ref_steps = plan_of(host), steps(host, m.n_rows)
    host.close()
    c = context(m, 3, upload=False)
    for on in (1, 0, 1, 1):
        c.set_option("ssor_plan_device", on)
        c.set_level_matrix(LEVEL, m)
        assert c.get_ssor_plan_origin(LEVEL) == (bool(on), 0, "")
        assert_same_plan(plan_of(c), ref_plan, on)
        assert all(np.array_equal(a, b) for a, b in zip(steps(c, m.n_rows), ref_steps))
        if on:
            c._chk(c.L.gmg_reset(c.h, C.c_int(2)))
            with pytest.raises(A.GMGError):
                c.get_ssor_plan_origin(LEVEL)
            c.set_level_matrix(LEVEL, m)
            assert c.get_ssor_plan_origin(LEVEL)[0]
            assert_same_plan(plan_of(c), ref_plan, "after reset")
    c.close()


def free_bytes():
    """free memory of device 0 as the HIP runtime reports it (the runtime the library itself is linked against)"""
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def free_after_rounds(one_round, rounds=6):
    free = []
    for _ in range(rounds):
        one_round()
        free.append(free_bytes())
    print("free device memory after each round, relative to the first:", [f - free[0] for f in free])
    return free


def test_no_leak_over_six_rounds():
    cases = [spc.lattice27(9), spc.tridiagonal(200), spc.wide_lower(), spc.unsorted()]

    def one_round():
        for m in cases:   # device-built plans and both kinds of fallback (before and after the kernels ran)
            c = context(m, 3, device=True)
            c.set_option("sgs_y_slots", 64)
            c.set_level_matrix(LEVEL, m)
            c.close()

    free = free_after_rounds(one_round)
    assert free[-1] == free[0], free


def test_a_refused_call_leaves_the_level_empty():
    """block rows that do not end at n_rows: refused before anything is planned, with the option as without it"""
    A = capi()
    m = spc.lattice27(9)
    c = context(m, 1, device=True)
    c.set_ssor_block_rows(LEVEL, [0, 5, m.n_rows - 1])
    c._chk(c.L.gmg_reset(c.h, C.c_int(2)))
    with pytest.raises(A.GMGError) as e:
        c.set_level_matrix(LEVEL, m)
    assert e.value.code == A.ERR_INVALID
    for f in (c.get_ssor_plan_origin, c.get_ssor_plan, lambda l: c.get_ssor_plan_array(l, "stream")):
        with pytest.raises(A.GMGError):
            f(LEVEL)
    c.set_ssor_block_rows(LEVEL, [])
    c.set_level_matrix(LEVEL, m)   # the context survives
    assert c.get_ssor_plan_origin(LEVEL) == (True, 0, "")
    c.close()


# ------------------------------------------------------------------------------------------------ whole runs of the driver

ALL_RESIDENT = dict(mesh_tables_on_device=True, system_matrix_on_device=True, level_matrices_on_device=True, rhs_from_cell_tables=True,
                    operators_from_resident_tables=True, estimator_on_device=True, analytical_on_device=True, refinement_on_device=True,
                    transfer_on_device=True, densities_on_device=True, densities_from_resident_tables=True, estimator_from_resident_tables=True,
                    energy_forces_from_resident_tables=True, compute_forces=True, energy_for_large_systems=True, short_range_cutoff=2.5)


def atoms_problem(n_atoms, cycles, key, **more):
    import energy_resident_cases as erc
    from gpu_util import pkg

    S = pkg().step50
    right, vacuum, data = {8: (1.0, 10, erc.GOLDEN_8), 216: (3.0, 2, erc.GOLDEN_216)}[n_atoms]
    p = S.Problem(S.prm_text(left=0, right=right, mesh_size=0.25, vacuum=vacuum, problem="GaussianCharges", dim=3, bc="Inhomogeneous", cycles=cycles, r_c=0.5,
                             cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR", refinement_estimator="Kelly",
                             ssor_plan_on_device=key, **more))
    p.read_lammps(data)
    return p


def step16_3d(cycles, key):
    from test_coef_matrix_cpu import step16_problem
    return step16_problem(3, 2, cycles, smoother="SSOR", level_matrices_on_device=True, ssor_plan_on_device=key)


DRIVER_RUNS = {"8-atoms-3-cycles-1-block": (lambda key: atoms_problem(8, 3, key, ssor_blocks=1), 3, False),
               "8-atoms-3-cycles-4-blocks": (lambda key: atoms_problem(8, 3, key, ssor_blocks=4, level_matrices_on_device=True), 3, True),
               "216-atoms-2-cycles-resident": (lambda key: atoms_problem(216, 2, key, **ALL_RESIDENT), 2, True),
               "step16-3d-2-cycles": (lambda key: step16_3d(2, key), 2, True)}


@pytest.mark.parametrize("run", sorted(DRIVER_RUNS))
def test_driver_runs_with_the_key_off_and_on(run, monkeypatch):
    """logs, iteration counts, marks and solution bits of whole runs; with the key every level >= 1 is planned on the device
    (checked by the driver against a host-planned second build: STEP50_CHECK_RESIDENT) and, where the device assembled the
    level, no byte of col / val came back"""
    monkeypatch.setenv("STEP50_CHECK_RESIDENT", "1")
    make, cycles, assembled = DRIVER_RUNS[run]
    out = {}
    for key in (False, True):
        p = make(key)
        got = []
        for cycle in range(cycles):
            rep = p.run_cycle(cycle, on_device=True)
            got.append((rep["cg_iterations"], rep["coarse_iterations"], p.vector("solution").view(np.uint64).tolist(), np.asarray(p.marks()).tolist()))
            for l in range(1, p.n_levels()):
                on_device, moved, why = p.ssor_plan_origin(l)
                assert (on_device, why) == (key, ""), (run, key, cycle, l, why)
                assert moved == 0 if key or not assembled else moved > 0, (run, key, cycle, l, moved)
        log = [line for line in p.log().splitlines() if "seconds" not in line and " ms" not in line]
        assert not any("SSOR plan on device" in line for line in log)
        if "resident" in run:
            assert not any("not applicable" in line for line in log), [line for line in log if "not applicable" in line]
        out[key] = (got, log)
        p.close()
    assert out[False][1] == out[True][1]
    assert out[False][0] == out[True][0]


def test_driver_on_a_communicator_says_once_why_the_host_planned():
    """one rank on a communicator, two cycles, several levels: the line appears exactly once, and the run is the one without the key"""
    out = []
    for key in (False, True):
        p = atoms_problem(8, 2, key)
        p.set_communicator(0, 1, capi().Context.unique_id())
        got = []
        for cycle in range(2):
            rep = p.run_cycle(cycle, on_device=True)
            got.append((rep["cg_iterations"], p.vector("solution").view(np.uint64).tolist()))
        assert p.n_levels() >= 2
        for l in range(1, p.n_levels()):
            assert p.ssor_plan_origin(l) == (False, 0, "communicator" if key else "")
        assert p.log().count("SSOR plan on device: not applicable (communicator), planned on the host") == int(key)
        out.append(got)
        p.close()
    assert out[0] == out[1]
