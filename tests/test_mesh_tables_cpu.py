"""DoF numbering, constraint lines and level flags restated from the forest alone (tests/mesh_tables_reference.py: the
definitions of gmg_build_mesh_tables) against the host driver's distribute_dofs and make_constraints (src/step-50.cc:661-706:
dof_handler.distribute_dofs / distribute_mg_dofs, make_hanging_node_constraints, interpolate_boundary_values, close,
MGConstrainedDoFs), exactly, on the meshes of tests/mesh_tables_cases.py; and what "Mesh tables on device" does to a cycle that
does not run on the device.  Needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import mesh_tables_cases as mtc
import mesh_tables_reference as mtr
from gpu_util import capi, pkg


@pytest.mark.parametrize("name", sorted(mtc.CASES))
def test_reference_equals_host(name):
    x = mtc.case(name)
    r, inp = x.ref, x.sys
    nv = 1 << x.fc.dim
    assert r.n_dofs == inp.n_dofs and r.n_cells == len(inp.cell_level)
    assert np.array_equal(np.asarray(r.cell_dofs, dtype=np.int32).reshape(-1, nv), inp.cell_dofs)
    assert np.array_equal(np.asarray(r.cell_level, dtype=np.uint8), inp.cell_level)
    assert np.array_equal(np.asarray(r.constraint_of_dof, dtype=np.int32), inp.constraint_of_dof)
    assert r.n_lines == len(inp.line_inhomogeneity)
    # the hanging lines whose masters are all free are stored as built: masters in corner order, weights 1 / m
    cons = r.constraint_of_dof
    for l in range(r.n_hanging):
        a, b = r.line_ptr[l], r.line_ptr[l + 1]
        if all(cons[m] < 0 for m in r.line_master[a:b]):
            ha, hb = int(inp.line_ptr[l]), int(inp.line_ptr[l + 1])
            assert inp.line_master[ha:hb].tolist() == r.line_master[a:b] and inp.line_weight[ha:hb].tolist() == r.line_weight[a:b], (name, l)
    # the same close() on the reference's lines, with the host's boundary values: the whole tables
    ptr, master, weight, inhom = mtr.close(r, inp.line_inhomogeneity[r.n_hanging:].tolist())
    assert ptr == inp.line_ptr.tolist() and master == inp.line_master.tolist()
    assert np.array_equal(np.asarray(weight, dtype=np.float64).view(np.uint64), inp.line_weight.view(np.uint64))
    assert np.array_equal(np.asarray(inhom, dtype=np.float64).view(np.uint64), inp.line_inhomogeneity.view(np.uint64))
    # every level: the cell table and the flags
    assert len(r.levels) == len(x.levels) == x.fc.n_levels
    for l, (rl, hl) in enumerate(zip(r.levels, x.levels)):
        assert rl.n_dofs == hl.n_dofs, (name, l)
        assert np.array_equal(np.asarray(rl.cell_dofs, dtype=np.int32).reshape(-1, nv), hl.cell_dofs), (name, l)
        assert np.array_equal(np.asarray(rl.dof_flags, dtype=np.uint8), hl.dof_flags), (name, l)
    # vertex_of_dof: Forest::vertex_coords of the reference's keys is dof_coordinates(), bit for bit
    hf = x.h0 / 4096.0
    want = np.zeros((r.n_dofs, 3))
    for i, key in enumerate(r.vertex_of_dof):
        v = mtr.unpack(key)
        for d in range(x.fc.dim):
            want[i, d] = x.origin + hf * float(v[d])
    assert np.array_equal(want.view(np.uint64), x.xyz.view(np.uint64))


def _content(name):
    x = mtc.case(name)
    r, dim = x.ref, x.fc.dim
    n0 = x.fc.n0.tolist()
    m = [r.line_ptr[l + 1] - r.line_ptr[l] for l in range(r.n_hanging)]
    edge_levels = [l for l, lv in enumerate(r.levels) if any(f & 2 for f in lv.dof_flags)]
    return dict(dim=dim, face=sum(1 for k in m if k == 4), edge=sum(1 for k in m if k == 2), revisits=r.n_visits - r.n_hanging,
                hanging_on_boundary=sum(1 for l in range(r.n_hanging) if mtr.on_boundary(dim, n0, r.vertex_of_dof[r.line_dof[l]])),
                dirichlet=r.n_lines - r.n_hanging, edge_dofs=sum(1 for lv in r.levels for f in lv.dof_flags if f & 2),
                upper_levels_without_edge=[l for l in range(1, len(r.levels)) if l not in edge_levels], lexicographic=x.fc.level0_lexicographic)


def test_cases_cover_what_the_comparison_is_about():
    """face-centre and edge lines, an edge mid-point reached by more than one face, a hanging node on the boundary,
    refinement-edge DoFs and an upper level without them, both dimensions, both level-0 numberings, and a mesh without hanging
    nodes: without them the comparisons prove nothing"""
    got = {name: _content(name) for name in mtc.CASES}
    print(got)
    assert got["G8-c0"]["face"] == got["G8-c0"]["edge"] == 0 and got["G8-c0"]["dirichlet"] > 0
    for name in ("A3", "B3", "G8-c1", "G8-c2", "S3-c1", "CW-c1"):
        assert got[name]["face"] > 0 and got[name]["edge"] > 0 and got[name]["revisits"] > 0 and got[name]["edge_dofs"] > 0, name
    for name in ("S2-c1", "S2-c2"):
        assert got[name]["dim"] == 2 and got[name]["face"] == 0 and got[name]["edge"] > 0 and got[name]["edge_dofs"] > 0, name
    assert got["A3"]["hanging_on_boundary"] > 0                       # A3 refines up to the boundary
    assert got["S2-c1"]["upper_levels_without_edge"][:3] == [1, 2, 3]  # the globally refined levels
    assert got["S3-c1"]["upper_levels_without_edge"][:2] == [1, 2]
    assert not got["CW-c1"]["lexicographic"] and got["G8-c1"]["lexicographic"]


def test_hand_built_forests():
    q = mtr.build(mtr.quadrant_2d())
    # the active cells: the coarse cells (1,0), (0,1), (1,1), then the four children of (0,0); 8 coarse + 2 fine vertices on the boundary
    assert (q.n_cells, q.n_dofs, q.n_hanging, q.n_lines) == (7, 14, 2, 12) and q.cell_level == [0, 0, 0, 1, 1, 1, 1]
    assert q.cell_dofs[:4] == [[0, 1, 2, 3], [4, 2, 5, 6], [2, 3, 6, 7], [8, 9, 10, 11]] and q.cell_dofs[4] == [9, 0, 11, 12]
    # cell (1,0) meets the mid-point of its face x = 1 first, cell (0,1) the mid-point of its face y = 1: masters in corner order
    assert [q.line_master[q.line_ptr[l]:q.line_ptr[l + 1]] for l in range(2)] == [[0, 2], [4, 2]] and q.line_weight == [0.5] * 4
    assert [mtr.unpack(q.vertex_of_dof[d])[:2] for d in q.line_dof[:2]] == [[4096, 2048], [2048, 4096]]
    assert q.line_dof[:2] == [12, 13] and q.line_dof[2:] == [0, 1, 3, 4, 5, 6, 7, 8, 9, 10] and q.line_ptr == [0, 2] + [4] * 11
    assert q.levels[0].dof_flags == [1, 1, 1, 1, 0, 1, 1, 1, 1] and q.levels[0].cell_dofs[3] == [4, 5, 7, 8]
    # level 1 in first-touch order: (1,0) and (0,1) of the root lattice lie on the boundary and on the refinement edge
    assert q.levels[1].dof_flags == [1, 1, 1, 0, 3, 2, 3, 2, 2]
    qc = mtr.build(mtr.quadrant_2d(False))
    assert qc.levels[0].cell_dofs == [[0, 1, 2, 3], [1, 4, 3, 5], [2, 3, 6, 7], [3, 5, 7, 8]] and qc.cell_dofs == q.cell_dofs
    e = mtr.build(mtr.edge_only_3d())
    assert (e.n_cells, e.n_hanging) == (11, 9) and e.n_visits == 10   # the mid-point of the edge x = y = 1 is met from cells (1,0,0) and (0,1,0)
    shared = [l for l in range(e.n_hanging) if mtr.unpack(e.vertex_of_dof[e.line_dof[l]]) == [4096, 4096, 2048]]
    assert len(shared) == 1
    masters = e.line_master[e.line_ptr[shared[0]]:e.line_ptr[shared[0] + 1]]
    # its masters are the two ends of the edge, which all three coarse cells share -- (1,1,0) too, that touches the refined cell there only
    assert masters == [2, 6] and set(masters) == set(e.cell_dofs[0]) & set(e.cell_dofs[1]) & set(e.cell_dofs[2])
    s = mtr.build(mtr.single_cell(3))
    assert (s.n_cells, s.n_dofs, s.n_hanging, s.n_lines) == (1, 8, 0, 8) and s.levels[0].dof_flags == [1] * 8
    z = mtr.build(mtr.empty(2))
    assert (z.n_cells, z.n_dofs, z.n_lines, z.line_ptr) == (0, 0, 0, [0]) and z.levels[0].n_dofs == 0
    with pytest.raises(mtr.Unbalanced):
        mtr.build(mtr.unbalanced_2d())


def test_key_defaults_to_the_host_loops():
    """without the key nothing changes; with it, a cycle that does not run on the device says so once and keeps the host path"""
    S = pkg().step50
    args = dict(left=-1, right=1, mesh_size=0.25, vacuum=1, problem="GaussianCharges", dim=2, bc="Homogeneous", cycles=1, r_c=0.5, global_refinement=0)
    p = S.Problem(S.prm_text(**args))
    p.run_cycle(0, on_device=False)
    assert not p.mesh_tables_on_device() and "Mesh tables on device" not in p.log()
    q = S.Problem(S.prm_text(mesh_tables_on_device=True, **args))
    q.run_cycle(0, on_device=False)
    assert not q.mesh_tables_on_device() and q.log().count("Mesh tables on device: not applicable (the cycle does not run on the device)") == 1
    a, b = p.system_assembly_inputs(), q.system_assembly_inputs()
    assert np.array_equal(a.cell_dofs, b.cell_dofs) and np.array_equal(a.constraint_of_dof, b.constraint_of_dof)
    assert "mesh_tables_on_device" not in S.prm_text(**args) and "set Mesh tables on device = true" in S.prm_text(mesh_tables_on_device=True)
    fc = p.forest_cells()
    assert fc.dim == 2 and fc.n_levels == 1 and fc.level_ptr.tolist() == [0, fc.n0[0] * fc.n0[1]] and fc.n0[2] == 1 and np.all(fc.cell_first_child == -1)
    p.close()
    q.close()


def test_null_context_is_refused():
    L = capi().load()
    assert L.gmg_build_mesh_tables(None, C.c_int(3), None, C.c_int(0), None, None, None, C.c_int(0), None) == capi().ERR_INVALID
    assert L.gmg_get_mesh_tables(None, *([None] * 13)) == capi().ERR_INVALID
    assert L.gmg_get_mesh_level_tables(None, C.c_int(0), None, None, None, None, None) == capi().ERR_INVALID
