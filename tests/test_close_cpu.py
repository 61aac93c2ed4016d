"""tests/close_reference.py -- the definition of gmg_close_constraints in plain loops -- pinned against the host driver's closed
constraint_lines (LaplaceProblem::make_constraints, "close()"), exactly: entries, their order, the bits of the weights and of
the inhomogeneities.  The unclosed input: the driver closes its constraint_lines in place inside make_constraints and exports
only the closed lines (Problem.system_assembly_inputs), so its own unclosed lines cannot be read back.  What stands in for them
is the restatement of tests/mesh_tables_reference.py on the cycle's forest, which tests/test_mesh_tables_cpu.py holds against the
host exactly: the numbering, constraint_of_dof, the number of lines and every hanging line that close() leaves as built.
test_unclosed_input_is_the_hosts here adds the rest, so that the input is pinned to the host on its own: every closed host
line is the reference's unclosed line with exactly the entries whose master carries a Dirichlet line removed, in order, with
the same weights.  The Dirichlet values are the host's.  Needs no GPU."""
import numpy as np
import pytest

import close_reference as cr
import mesh_tables_cases as mtc

#  A3 / B3: tests/mg_cases.py (B3: Inhomogeneous, nonzero boundary values); G8: the golden 8-atom run, cycles 1 and 2; S2-c2: Step16
#  in 2D refined twice; S3-c1: Step16 in 3D, cycle 1
CASES = ("A3", "B3", "G8-c1", "G8-c2", "S2-c2", "S3-c1")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_lines(got, host, what=""):
    """closed lines (lists or arrays) against the host's line tables of Problem.system_assembly_inputs()"""
    assert np.array_equal(np.asarray(got.line_ptr, dtype=np.int64), host.line_ptr), (what, "line_ptr")
    assert np.array_equal(np.asarray(got.line_master, dtype=np.int32), host.line_master), (what, "line_master")
    assert np.array_equal(bits(got.line_weight), bits(host.line_weight)), (what, "line_weight")
    assert np.array_equal(bits(got.line_inhomogeneity), bits(host.line_inhomogeneity)), (what, "line_inhomogeneity")
    return True


def dirichlet_values(x):
    return x.sys.line_inhomogeneity[x.ref.n_hanging:]


@pytest.mark.parametrize("name", CASES)
def test_reference_equals_host(name):
    x = mtc.case(name)
    assert same_lines(cr.close_tables(x.ref, dirichlet_values(x).tolist()), x.sys, name)


@pytest.mark.parametrize("name", CASES)
def test_unclosed_input_is_the_hosts(name):
    """the reference's unclosed lines restricted to unconstrained masters are the host's closed entries, line by line (no
    arithmetic: this pins the input of close_reference independently of close_reference)"""
    x = mtc.case(name)
    r, h = x.ref, x.sys
    assert np.array_equal(np.asarray(r.constraint_of_dof, dtype=np.int32), h.constraint_of_dof) and r.n_lines == len(h.line_inhomogeneity)
    for l in range(r.n_lines):
        a, b = r.line_ptr[l], r.line_ptr[l + 1]
        free = [(m, w) for m, w in zip(r.line_master[a:b], r.line_weight[a:b]) if r.constraint_of_dof[m] < 0]
        ha, hb = int(h.line_ptr[l]), int(h.line_ptr[l + 1])
        assert [m for m, _ in free] == h.line_master[ha:hb].tolist() and [w for _, w in free] == h.line_weight[ha:hb].tolist(), (name, l)
        assert all(r.constraint_of_dof[m] >= r.n_hanging for m in r.line_master[a:b] if r.constraint_of_dof[m] >= 0), (name, l)


def content(name):
    x = mtc.case(name)
    r = x.ref
    values = dirichlet_values(x)
    lost_nonzero = lost_two = keeps_all = 0
    for l in range(r.n_hanging):
        ms = [r.constraint_of_dof[m] for m in r.line_master[r.line_ptr[l]:r.line_ptr[l + 1]]]
        dropped = [m for m in ms if m >= r.n_hanging]
        lost_nonzero += any(values[m - r.n_hanging] != 0.0 for m in dropped)
        lost_two += len(dropped) == 2
        keeps_all += not dropped
    return dict(dim=x.fc.dim, lost_nonzero=lost_nonzero, lost_two=lost_two, keeps_all=keeps_all, hanging=r.n_hanging)


def test_cases_cover_what_the_comparison_is_about():
    got = {name: content(name) for name in CASES}
    print(got)
    assert any(c["lost_nonzero"] > 0 for c in got.values())   # an entry folded into a nonzero boundary value
    assert any(c["lost_two"] > 0 for c in got.values())
    assert all(c["keeps_all"] > 0 for c in got.values())
    assert {c["dim"] for c in got.values()} == {2, 3}


def test_hand_built_tables():
    # DoFs 0 .. 5; line 0 (hanging, DoF 4): masters 0, 1; line 1 (hanging, DoF 5): masters 1, 2, 3, 0; lines 2, 3: Dirichlet on DoFs 1 and 3
    cons = [-1, 2, -1, 3, 0, 1]
    ptr, master, weight = [0, 2, 6, 6, 6], [0, 1, 1, 2, 3, 0], [0.5, 0.5, 0.25, 0.25, 0.25, 0.25]
    c = cr.close(cons, ptr, master, weight, 2, 4, [3.0, -0.1])
    assert c.line_ptr == [0, 1, 3, 3, 3] and c.line_master == [0, 2, 0] and c.line_weight == [0.5, 0.25, 0.25]
    assert c.line_inhomogeneity == [0.0 + 0.5 * 3.0, (0.0 + 0.25 * 3.0) + 0.25 * -0.1, 3.0, -0.1]
    z = cr.close(cons, ptr, master, weight, 2, 4)   # no values: all +0.0
    assert z.line_ptr == c.line_ptr and z.line_inhomogeneity == [0.0] * 4 and all(np.signbit(z.line_inhomogeneity) == 0)
    # a hanging master raises
    with pytest.raises(cr.HangingMaster):
        cr.close([-1, -1, 0, 1], [0, 2, 4], [0, 1, 2, 0], [0.5] * 4, 2, 2, [])
    # zero lines
    e = cr.close([-1, -1], [0], [], [], 0, 0, [])
    assert e.line_ptr == [0] and e.line_master == [] and e.line_inhomogeneity == []
    # all Dirichlet
    d = cr.close([0, 1, 2], [0, 0, 0, 0], [], [], 0, 3, [1.0, 2.0, -0.0])
    assert d.line_ptr == [0, 0, 0, 0] and d.line_inhomogeneity[:2] == [1.0, 2.0] and np.signbit(d.line_inhomogeneity[2])
    with pytest.raises(ValueError):
        cr.close([0, 1, 2], [0, 0, 0, 0], [], [], 0, 3, [1.0])
