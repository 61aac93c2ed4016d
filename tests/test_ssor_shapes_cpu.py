"""The record shapes of the four-wave SSOR sweep without a GPU: tests/ssor_plan_replay.cc, in its file mode,
plans every matrix of tests/ssor_shape_cases.py under seven option sets, decodes every record, replays a forward and a backward
sweep bit for bit and prints which shapes (g, l1, l2) the plan holds, per direction and plan kind.  Asserted here: the replay
passes; every case holds the (shape, direction) pairs it was chosen for; the union over the default plans holds the floor of 38
shapes and the union over all option sets six more; the mesh matrices of the other SSOR tests hold the shapes recorded for them;
and a stride or a T1 / T2 boundary decoded wrongly for ONE shape is noticed by exactly the plans that hold that shape."""
import pytest

import ssor_plan_cases as spc
import ssor_shape_cases as K

CASE_NAMES = [c.name for c in K.CASES]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return K.build_replay(tmp_path_factory.mktemp("ssor_shapes"))


MUTATION_SETS = ("default", "chunk-1", "reg")   # lane-major records with one shape per chunk and per step, field-major records


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the case files, written once: all option sets, and the three the decode mutations run under"""
    d = tmp_path_factory.mktemp("ssor_shape_files")
    out = {}
    for c in K.CASES:
        m, bounds = c.make()
        out[c.name] = d / c.name
        K.write_case(out[c.name], m, c.blocks, bounds)
        out[c.name, "mutations"] = d / (c.name + "-mutations")
        K.write_case(out[c.name, "mutations"], m, c.blocks, bounds, {k: K.OPTION_SETS[k] for k in MUTATION_SETS})
    return out


@pytest.fixture(scope="module")
def replays(exe, files):
    """every case replayed once under every option set: read-only"""
    return {name: K.replay(exe, files[name]) for name in CASE_NAMES}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_matrix_is_what_the_cases_promise(name):
    m, bounds = K.case(name).make()
    assert 128 <= m.n_rows <= 620 and int((m.rowptr[1:] - m.rowptr[:-1]).max()) <= 72
    pattern, off = set(), []
    for i in range(m.n_rows):
        cols = m.col[m.rowptr[i]:m.rowptr[i + 1]]
        assert all(a < b for a, b in zip(cols, cols[1:])) and i in cols
        vals = m.val[m.rowptr[i]:m.rowptr[i + 1]]
        assert vals[cols == i][0] > abs(vals[cols != i]).sum()   # dominant diagonal
        pattern |= {(i, int(c)) for c in cols}
        off += [float(v) for v, c in zip(vals, cols) if c != i]
    assert all((j, i) in pattern for i, j in pattern)
    assert len(set(off)) == len(off) and all(1.0 <= -v <= 2.0 for v in off)   # distinct, of comparable size
    if bounds:
        assert bounds[0] == 0 and bounds[-1] == m.n_rows and all(a <= b for a, b in zip(bounds, bounds[1:]))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_replay_passes_and_the_case_holds_its_pairs(replays, name):
    c = K.case(name)
    status, plans, tables, err = replays[name]
    assert status == 0 and set(plans) == set(K.OPTION_SETS), err
    assert all(p["failures"] == 0 for p in plans.values())
    assert set(c.pairs) <= K.pairs_of(tables["default"]), sorted(set(c.pairs) - K.pairs_of(tables["default"]))
    for key, want in c.expect.items():
        got = max(K.direction_entries(c.make()[0])) if key == "entries" else plans["default"][key]
        assert got >= want if key == "switches" else got == want, (key, got, want)
    # the plan kinds are what the option sets ask for (a plan that fell back to the one-wave sweep has neither)
    for name_, p in plans.items():
        if p["phased"]:
            assert p["dep"] == (name_ == "dep") and p["reg"] == (name_ == "reg")
            assert (p["self_ranges"] == 0) if name_ in ("sliding-off", "dep", "reg") else True
    assert not plans["default"]["phased"] or plans["default"]["self_ranges"] == plans["default"]["ranges"]


def test_partitions_and_step_sizes_are_covered(replays):
    """B = 1, B = 3 and a caller-given partition with an empty block; a step of 32 rows and a step of one row; 36 entries in a
    direction planned, 37 on the one-wave plan; steps that change shape inside a range"""
    assert {c.blocks for c in K.CASES} >= {1, 3}
    assert any(bounds and any(a == b for a, b in zip(bounds, bounds[1:])) for bounds in (c.make()[1] for c in K.CASES))
    rows = [(p["default"]["min_rows"], p["default"]["max_rows"]) for _, p, _, _ in replays.values() if p["default"]["phased"]]
    assert min(r[0] for r in rows) == 1 and max(r[1] for r in rows) == 32
    assert replays["36-lower-neighbours"][1]["default"]["phased"] == 1 and replays["37-lower-neighbours"][1]["default"]["retried"] == 1
    assert replays["alternating"][1]["default"]["switches"] >= 2


def test_floor_of_shapes(replays):
    default = set().union(*[K.pairs_of(t["default"]) for _, _, t, _ in replays.values()])
    every = set().union(*[K.pairs_of(table) for _, _, t, _ in replays.values() for table in t.values()])
    assert set(K.FLOOR_DEFAULT) <= {p[:3] for p in default}, sorted(set(K.FLOOR_DEFAULT) - {p[:3] for p in default})
    assert set(K.FLOOR_DEFAULT + K.FLOOR_OPTIONS) <= {p[:3] for p in every}
    forward, backward = ({p[:3] for p in default if p[3] == d} for d in (0, 1))
    print(f"[ssor-shapes] default plan: {len(forward)} shapes forward, {len(backward)} backward, {len(forward | backward)} of {len(K.ALL_SHAPES)}; "
          f"unreached forward {sorted(set(K.ALL_SHAPES) - forward)} backward {sorted(set(K.ALL_SHAPES) - backward)}; "
          f"all option sets: {len(every)} (shape, direction) pairs")
    assert set(K.PAIRS) <= set(CASE_NAMES)   # (every recorded list belongs to a case)


MESHES = {"lattice27-9": lambda: spc.lattice27(9), "lattice27-17": lambda: spc.lattice27(17)}
MESHES.update({f"{name}-level{l + 1}": (lambda name, l: lambda: spc.adaptive_levels(name)[l])(name, l) for name in ("A3", "B3") for l in range(2)})


@pytest.mark.parametrize("mesh,blocks", list(K.MESH_PLANS), ids=[f"{m}-B{b}" for m, b in K.MESH_PLANS])
def test_mesh_matrices_hold_the_recorded_shapes(exe, tmp_path, mesh, blocks):
    """The statement of the gap: which shapes the mesh matrices of the other SSOR tests select, so that a change of the cost
    model that moves them onto other shapes is noticed here.  The reference is the one DESIGN.md section 32 names: the default
    plan of ssor_sweep_plan, shape keys read from blk_tab, recorded per matrix and block count in K.MESH_PLANS and compared for
    equality.  The 27-point lattices hold only the six shapes of K.MESH_SHAPES, exactly as tabulated there (9 cubed with B = 1 two
    of them, with B = 3 four; 17 cubed three).  The adaptive levels A3 / B3 do NOT stay inside the six, as the section first
    assumed: their hanging-node and boundary rows select eleven more, so the existing GPU tests ran 17 of the 51 shapes."""
    K.write_case(tmp_path / "mesh", MESHES[mesh](), blocks, (), {"default": ()})
    status, plans, tables, err = K.replay(exe, tmp_path / "mesh")
    assert status == 0 and plans["default"]["phased"] == 1, err
    seen = {p[:3] for p in K.pairs_of(tables["default"])}
    assert seen == set(K.MESH_PLANS[mesh, blocks]), (sorted(seen - set(K.MESH_PLANS[mesh, blocks])), sorted(set(K.MESH_PLANS[mesh, blocks]) - seen))
    if mesh.startswith("lattice27"):
        assert seen <= set(K.MESH_SHAPES)


def test_the_gap_is_what_the_meshes_leave():
    """the six shapes are the lattices' and all six occur; all mesh matrices together hold 17 shapes, so 34 of the 51 ran on no GPU
    before the cases of this file (which hold all 51: test_floor_of_shapes and the pairs of the cases)"""
    lattices = set().union(*[set(v) for (m, _), v in K.MESH_PLANS.items() if m.startswith("lattice27")])
    meshes = set().union(*[set(v) for v in K.MESH_PLANS.values()])
    assert lattices <= set(K.MESH_SHAPES) <= meshes <= set(K.ALL_SHAPES)
    assert len(meshes) == 17 and len(set(K.ALL_SHAPES) - meshes) == 34
    held = set().union(*[{p[:3] for p in c.pairs} for c in K.CASES])
    assert set(K.ALL_SHAPES) - meshes <= held


@pytest.mark.parametrize("kind", ["stride", "t1"])
def test_a_wrongly_decoded_shape_is_noticed_by_exactly_the_plans_that_hold_it(exe, files, replays, kind):
    """the case set separates the shapes: decoding the records of one shape with a stride 32 bytes too long, or with T1 ending
    four slots late, fails in every plan that holds the shape (under each of MUTATION_SETS) and in no other"""
    mutations = [(K.shape_key(*s), kind) for s in K.ALL_SHAPES]
    noticed = set()
    for name in CASE_NAMES:
        tables = replays[name][2]
        got = K.replay_mutations(exe, files[name, "mutations"], mutations)
        for shape, mutation in zip(K.ALL_SHAPES, mutations):
            for option_set in MUTATION_SETS:
                table = tables[option_set]
                holds = shape in {k[:3] for k in table}
                assert (got[mutation][option_set] > 0) == holds, (name, option_set, shape, kind, got[mutation][option_set])
                if holds:
                    noticed.add(shape)
    assert noticed >= set(K.FLOOR_DEFAULT + K.FLOOR_OPTIONS)
