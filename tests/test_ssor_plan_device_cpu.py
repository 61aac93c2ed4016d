"""Option ssor_plan_device / prm key "SSOR plan on device"  as far as they show without a GPU: the two
new entries exist, the option's key is known to the library and documented, the prm key defaults to false, and a cycle that
runs on the host prints the same log with the key as without it.  The cases of tests/ssor_plan_cases.py are checked for what
they claim to exercise."""
import os

import numpy as np

import ssor_plan_cases as spc
from gpu_util import capi, pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_new_symbols_exist():
    lib = capi().load()
    for name in ("gmg_get_ssor_plan_array", "gmg_get_ssor_plan_origin"):
        assert name in capi().SYMBOLS and hasattr(lib, name)
    assert hasattr(pkg().step50.load(), "step50_ssor_plan_origin")
    assert len(capi().SSOR_PLAN_ARRAYS) == 10


def test_the_option_key_is_known_and_documented():
    """(no context without a GPU: gmg_set_option itself is exercised by tests/test_gpu_ssor_plan_device.py)"""
    lib_path = capi().load()._name
    with open(lib_path, "rb") as f:
        assert b"ssor_plan_device" in f.read()
    with open(os.path.join(ROOT, "include", "gmg_coulomb.h")) as f:
        header = f.read()
    assert "ssor_plan_device" in header
    for k, name in enumerate(capi().SSOR_PLAN_ARRAYS):
        assert f"#define GMG_SSOR_PLAN_{name.upper() if name != 'ranges' else 'RANGES'} {k}\n" in header


def test_prm_key_defaults_to_false_and_a_host_cycle_prints_todays_log():
    S = pkg().step50
    args = dict(left=-1, right=1, mesh_size=0.25, vacuum=1, problem="GaussianCharges", dim=2, bc="Homogeneous", cycles=1, r_c=0.5, global_refinement=0,
                smoother="SSOR")
    assert "SSOR plan on device" not in S.prm_text(**args) and "set SSOR plan on device = true" in S.prm_text(ssor_plan_on_device=True)
    p = S.Problem(S.prm_text(**args))                              # the key left out: its default
    q = S.Problem(S.prm_text(ssor_plan_on_device=False, **args))   # the default spelled out
    r = S.Problem(S.prm_text(ssor_plan_on_device=True, **args))
    logs = []
    for x in (p, q, r):
        x.run_cycle(0, on_device=False)
        logs.append(x.log())
        x.close()
    assert logs[0] == logs[1] == logs[2] and "SSOR plan" not in logs[0]


def test_cases_exercise_what_they_claim():
    for c in spc.DEVICE_CASES:
        if c.name.startswith(("A3", "B3")):
            continue
        m = c.make()
        rows = np.repeat(np.arange(m.n_rows), np.diff(m.rowptr))
        assert np.all(np.diff(m.rowptr) <= 28)
        for dirn in (m.col < rows, m.col > rows):   # at most 13 entries per direction: the shape g = 0, l1 = 16 holds every row
            assert np.bincount(rows[dirn], minlength=m.n_rows).max(initial=0) <= 13, c.name
        d = np.zeros(m.n_rows)
        np.add.at(d, rows, np.where(m.col == rows, m.val, -np.abs(m.val)))
        assert np.all(d > 0), c.name   # diagonally dominant
        assert all(np.all(np.diff(m.col[m.rowptr[i]:m.rowptr[i + 1]]) > 0) for i in range(m.n_rows)), c.name
    r = spc.random_symmetric()
    rows = np.repeat(np.arange(r.n_rows), np.diff(r.rowptr))
    off = r.col != rows
    assert 0.15 < np.mean(r.val[off] == 0.0) < 0.25 and set(zip(rows[off], r.col[off])) == set(zip(r.col[off], rows[off]))
    ns = spc.nonsymmetric()
    rows = np.repeat(np.arange(ns.n_rows), np.diff(ns.rowptr))
    assert set(zip(rows, ns.col)) != set(zip(ns.col, rows))
    w = spc.wide_lower()
    assert np.diff(w.rowptr).max() == 41
    assert np.diff(spc.too_wide().rowptr).max() == 80
    u = spc.unsorted()
    assert any(np.any(np.diff(u.col[u.rowptr[i]:u.rowptr[i + 1]]) < 0) for i in range(u.n_rows))
    assert {c.expect for c in spc.FALLBACK_CASES} >= {"no shape", "row too wide", "unsorted columns", "block does not fit", "balanced partition"}
    assert {b for _, b in spc.runs(spc.DEVICE_CASES)} >= {1, 3, 20}
