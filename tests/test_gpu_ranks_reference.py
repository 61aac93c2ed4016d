"""The rank-parallel path on 2, 3 and 4 ranks against independent references: the collectives of
csrc/gmg_comm.hpp by themselves, the partitioned SpMV with its halo plans, the coarse CG on a partitioned level 0 (the peer
branch of csrc/gmg_dist.hpp), the outer CG on a partitioned system, and the smoothers and the V-cycle with the SSOR sweep split
among the ranks.

All of it runs over the peer transport with the ranks sharing the one GPU: RCCL refuses two ranks on one device, so RCCL with
more than one rank stays unexecuted, and so does everything between different devices.  Every rank is a fresh interpreter
running tests/rank_worker.py on one group of steps of tests/rank_cases.py; it writes what it computed to an .npz and judges
nothing.  A (group, N) is launched once per module and its results are shared by the tests that read them.

No tolerance is chosen here: exact equality for the all-gathers, the derived bounds gamma_n sum |x_i y_i| for the reductions and
gamma_(k+1) sum_j |a_ij x_j| per row for the products (tests/partition_reference.py), cg_reference.x_tolerance and the checks of
tests/test_gpu_coarse_cg.py for the solves, and the tolerances of tests/mg_cases.py for the smoothers and the V-cycle.
tests/test_partition_reference_cpu.py, tests/test_cg_reference_cpu.py and tests/test_mg_reference_cpu.py prove the cases
sensitive.  Each test prints its worst error / tolerance ("[ranks-gpu]", run with -s).

A launch that runs into its time limit, or a rank ended by a signal, ends the launches of this module: the remaining children
are killed, the boot segment is unlinked, and every later test that would need a launch fails saying so.  Nothing is retried."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import cg_reference as R
import partition_reference as PR
import rank_cases as RC
from gpu_util import capi
from test_gpu_coarse_cg import check, outer_check, same_bits

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TAU = 1e-10

_stopped = {"why": None}     # set by a launch that hung or was ended by a signal: no further launch in this module
_launched = {}               # (group, N) -> per-rank results, or the exception of the launch


def run_ranks(group, n_ranks, directory):
    """one launch: n_ranks children, each a fresh interpreter, waited for with the group's time limit"""
    if _stopped["why"]:
        pytest.fail(f"not launched: an earlier launch of this module {_stopped['why']}")
    env = dict(os.environ, GMG_COMM_TRANSPORT="peer", GMG_PEER_SLOT_MB="2")
    with pytest.MonkeyPatch.context() as mp:     # the id is made by this process: it names the transport
        mp.setenv("GMG_COMM_TRANSPORT", "peer")
        mp.setenv("GMG_PEER_SLOT_MB", "2")
        uid = capi().Context.unique_id()         # (loads the library here first: no two children ever build it at once)
    assert uid.startswith(b"GMGPEER:")
    boot = "/dev/shm" + uid[len(b"GMGPEER:"):].split(b"\0")[0].decode()
    outs = [os.path.join(directory, f"{group}_n{n_ranks}_rank{r}.npz") for r in range(n_ranks)]
    logs = [open(o + ".stderr", "w") for o in outs]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "rank_worker.py"), str(r), str(n_ranks), uid.hex(), group, outs[r]],
                              env=env, stderr=logs[r]) for r in range(n_ranks)]
    deadline = time.monotonic() + RC.group_timeout(group)
    codes = []
    try:
        for p in procs:
            try:
                codes.append(p.wait(timeout=max(0.1, deadline - time.monotonic())))
            except subprocess.TimeoutExpired:
                codes.append(None)
                break
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
        for f in logs:
            f.close()
        try:
            os.unlink(boot)  # rank 0 unlinks it on a clean exit
        except OSError:
            pass
    tails = {r: open(o + ".stderr").read()[-600:] for r, o in enumerate(outs)}
    if None in codes:
        _stopped["why"] = f"({group}, {n_ranks} ranks) ran into its time limit of {RC.group_timeout(group)} s"
    elif any(c < 0 or c in (134, 139) for c in codes):
        _stopped["why"] = f"({group}, {n_ranks} ranks) had a rank ended by a signal (return codes {codes})"
    if _stopped["why"]:
        pytest.fail(f"{_stopped['why']}; stderr of the ranks: {tails}")
    assert codes == [0] * n_ranks, (group, n_ranks, codes, tails)
    return [dict(np.load(o)) for o in outs]


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    """get(group, N) -> the list of the ranks' results; every (group, N) is launched once, one launch at a time"""
    directory = str(tmp_path_factory.mktemp("ranks"))

    def get(group, n_ranks):
        key = (group, n_ranks)
        if key not in _launched:
            try:
                if group.startswith("mg-"):
                    write_hierarchy(group.split("-")[1], directory)
                _launched[key] = run_ranks(group, n_ranks, directory)
            except BaseException as e:  # noqa: BLE001  (kept: the tests that share this launch fail the same way)
                _launched[key] = e
        if isinstance(_launched[key], BaseException):
            raise _launched[key]
        return _launched[key]

    return get


def say(what, **ratios):
    print(f"\n[ranks-gpu] {what}: error / tolerance max " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))


def joined(per_rank, key):
    return np.concatenate([r[key] for r in per_rank])


def same_on_all(per_rank, key):
    for r in per_rank[1:]:
        assert np.array_equal(r[key], per_rank[0][key], equal_nan=True), (key, r[key], per_rank[0][key])
    return per_rank[0][key]


def check_info(info, n_ranks, level0_partitioned, ring=None):
    info = json.loads(str(info))
    assert info["ranks"] == n_ranks and info["transport"] == "peer" and info["devices"] == 1, info
    assert info["level0_partitioned"] == level0_partitioned, info
    if ring is not None:
        assert info["ring_memory"] == ring, info


# ------------------------------------------------------------------------------------------------ a. collectives

@pytest.mark.parametrize("n_ranks", RC.RANKS)
def test_allgather(ranks, n_ranks):
    """gmg_vec_allgather (allgather_full, allgather_chunks, peer_send_kernel, peer_recv_kernel) for n_global = 1, N - 1, N,
    N + 1, 4097 and 70001: the last rank's slice is empty or shorter.  Six rounds of every size and a run of mixed sizes, each
    run enqueued back to back with other data every round: both payload parities, the acknowledgement wait of round seq - 2, a
    long message followed by a short one.  Every rank must hold exactly the concatenation."""
    per_rank = ranks("collectives", n_ranks)
    tag, n_checked = 0, 0
    for li, sizes in enumerate(RC.allgather_rounds(n_ranks)):
        for j, n in enumerate(sizes):
            want = RC.allgather_values(tag, n)
            for r, res in enumerate(per_rank):
                got = res[f"ag{li}_{j}"]
                assert got.shape == want.shape and np.array_equal(got, want), (n_ranks, n, li, j, r, int(np.sum(got != want)))
            tag += 1
            n_checked += 1
    empty = sum(PR.owned_range(n, n_ranks - 1, n_ranks)[0] == n for sizes in RC.allgather_rounds(n_ranks) for n in sizes)
    assert empty > 0
    print(f"\n[ranks-gpu] all-gather on {n_ranks} ranks: {n_checked} rounds equal to the concatenation on every rank ({empty} with an empty last slice)")


@pytest.mark.parametrize("n_ranks", RC.RANKS)
def test_reductions(ranks, n_ranks):
    """gmg_vec_dot and gmg_vec_norms (allreduce_sum / allreduce_max, peer_allreduce_kernel) on partitioned vectors of 1, 257 and
    70001 entries per rank against numpy.longdouble.  Bound: gamma_n sum |x_i y_i|, gamma_n = n u / (1 - n u), n the global
    length -- it holds for every order of the n - 1 additions; the same for l1.  For l2 the library returns the root of the
    sum of squares: (l2)^2 carries the sum's n roundings and twice the root's one, gamma_(n + 2) sum x_i^2, with the square
    taken in longdouble.  linf is exact.  Every rank returns the same bits (the sum runs in rank order)."""
    per_rank = ranks("collectives", n_ranks)
    ld = np.longdouble
    worst = {"dot": 0.0, "l1": 0.0, "l2^2": 0.0}
    for length in RC.REDUCE_LENGTHS:
        xs, ys = zip(*[RC.reduce_vectors(length, r) for r in range(n_ranks)])
        x, y = np.concatenate(xs).astype(ld), np.concatenate(ys).astype(ld)
        n = len(x)
        dots, norms = same_on_all(per_rank, f"dot{length}"), same_on_all(per_rank, f"norms{length}")
        for got, a, b in ((dots[0], x, y), (dots[1], x, x)):
            bound = float(PR.gamma(n) * np.sum(np.abs(a * b)))
            err = abs(float(ld(got) - np.sum(a * b)))
            worst["dot"] = max(worst["dot"], err / bound)
            assert err <= bound, (n_ranks, length, got, err, bound)
        l1, l2, linf = norms
        b1, b2 = float(PR.gamma(n) * np.sum(np.abs(x))), float(PR.gamma(n + 2) * np.sum(x * x))
        e1, e2 = abs(float(ld(l1) - np.sum(np.abs(x)))), abs(float(ld(l2) * ld(l2) - np.sum(x * x)))
        worst["l1"], worst["l2^2"] = max(worst["l1"], e1 / b1), max(worst["l2^2"], e2 / b2)
        assert e1 <= b1 and e2 <= b2, (n_ranks, length, e1, b1, e2, b2)
        assert linf == float(np.max(np.abs(x))), (n_ranks, length, linf)
    say(f"reductions on {n_ranks} ranks", **worst)


@pytest.mark.parametrize("n_ranks", RC.RANKS)
def test_interleaved_collectives(ranks, n_ranks):
    """halo exchange, dot, all-gather, norms, five times over on one context: 20 collectives of four kinds that share the round
    counter and the payload slots"""
    per_rank = ranks("collectives", n_ranks)
    m = RC.operator(RC.MIX_OPERATOR)
    n = m.n_rows
    ld = np.longdouble
    worst = {"halo": 0.0, "dot": 0.0, "norms": 0.0}
    for i, op in enumerate(RC.MIX_OPS):
        x = RC.mix_vector(i, n)
        if op == "halo":
            y, bound = PR.spmv_bound(m, x)
            err = np.abs(joined(per_rank, f"mix{i}").astype(ld) - y).astype(np.float64)
            worst["halo"] = max(worst["halo"], float(np.max(err / bound)))
            assert np.all(err <= bound), (n_ranks, i, int(np.argmax(err / bound)))
        elif op == "dot":
            a, b = x.astype(ld), RC.mix_vector(100 + i, n).astype(ld)
            got, bound = same_on_all(per_rank, f"mix{i}")[0], float(PR.gamma(n) * np.sum(np.abs(a * b)))
            err = abs(float(ld(got) - np.sum(a * b)))
            worst["dot"] = max(worst["dot"], err / bound)
            assert err <= bound, (n_ranks, i, err, bound)
        elif op == "allgather":
            want = RC.allgather_values(1000 + i, RC.MIX_GATHER)
            for res in per_rank:
                assert np.array_equal(res[f"mix{i}"], want), (n_ranks, i)
        else:
            a = x.astype(ld)
            l1, l2, linf = same_on_all(per_rank, f"mix{i}")
            e1, b1 = abs(float(ld(l1) - np.sum(np.abs(a)))), float(PR.gamma(n) * np.sum(np.abs(a)))
            e2, b2 = abs(float(ld(l2) * ld(l2) - np.sum(a * a))), float(PR.gamma(n + 2) * np.sum(a * a))
            worst["norms"] = max(worst["norms"], e1 / b1, e2 / b2)
            assert e1 <= b1 and e2 <= b2 and linf == float(np.max(np.abs(x))), (n_ranks, i)
    say(f"20 interleaved collectives on {n_ranks} ranks", **worst)


# ------------------------------------------------------------------------------------------------ b. partitioned SpMV

@pytest.mark.parametrize("n_ranks", RC.RANKS)
def test_partitioned_spmv(ranks, n_ranks):
    """gmg_spmv(GMG_SYSTEM) and gmg_spmv(0) on owned rows with their halo plans (import_ghosts, halo_exchange): one entry per
    neighbour, plane cuts of a lattice, a band wider than a chunk (three neighbours, non-adjacent ones, a pair of ranks that
    are no neighbours), two decoupled blocks (no neighbours at all: the ranks must stay in step with the rounds that follow)
    and a one-sided pattern (a rank that sends and receives nothing back).  Five vectors in a row per operator; every row
    against its numpy.longdouble sum with the bound gamma_(k+1) sum_j |a_ij x_j|, k the row's length."""
    per_rank = ranks("spmv", n_ranks)
    ld = np.longdouble
    worst = {}
    for name in RC.spmv_operators(n_ranks):
        m = RC.operator(name)
        for r, res in enumerate(per_rank):   # the plans the ranks set are the reference's
            loc = PR.localize(m, r, n_ranks)
            assert np.array_equal(res[f"{name}_plan"], np.concatenate([loc.neighbor_rank, loc.send_count, loc.recv_count]))
        if name == "wide" and n_ranks == 4:
            plans = [list(PR.localize(m, r, 4).neighbor_rank) for r in range(4)]
            assert any(len(p) == 3 for p in plans) and 3 not in plans[0] and 3 in plans[1]
        if name == "blocks":
            assert all(len(res["blocks_plan"]) == 0 for res in per_rank)
        X = RC.spmv_vectors(name)
        for i in range(RC.N_SPMV_VECTORS):
            y, bound = PR.spmv_bound(m, X[i])
            for which in ("sys", "lv"):
                err = np.abs(joined(per_rank, f"{name}_{which}{i}").astype(ld) - y).astype(np.float64)
                worst[name] = max(worst.get(name, 0.0), float(np.max(err / bound)))
                assert np.all(err <= bound), (n_ranks, name, which, i, int(np.argmax(err / bound)), float(np.max(err / bound)))
        # the reduction that follows on the same context
        xs, ys = zip(*[RC.reduce_vectors(257, r) for r in range(n_ranks)])
        a, b = np.concatenate(xs).astype(ld), np.concatenate(ys).astype(ld)
        got = same_on_all(per_rank, f"{name}_dot")[0]
        assert abs(float(ld(got) - np.sum(a * b))) <= float(PR.gamma(len(a)) * np.sum(np.abs(a * b))), (n_ranks, name)
    say(f"partitioned SpMV on {n_ranks} ranks", **worst)


# ------------------------------------------------------------------------------------------------ c. coarse CG

def coarse_result(per_rank, key):
    """(x joined, iterations, residual, return code): the scalars must be the same on every rank"""
    it, res, rc = same_on_all(per_rank, key + "_m")
    return joined(per_rank, key + "_x"), int(it), float(res), int(rc)


def coarse_check(got, ref, name, what):
    """the checks of tests/test_gpu_coarse_cg.py::check; returns |x - x_ref| / tolerance"""
    check(got, ref, "csr" if name in RC.RHS_SEED else name, what)   # (the tolerance on x is one for all operators of this size)
    return float(np.abs(got[0] - ref.x).max() / (RC.x_tolerance(name) * np.abs(ref.x).max()))


@pytest.mark.parametrize("n_ranks", RC.RANKS)
def test_coarse_cg_on_a_partitioned_level0(ranks, n_ranks):
    """gmg_coarse_solve on owned rows (the peer branch of coarse_solve_unfused: the direction kernel pushing halo entries into
    the neighbours' ring, peer_wait_halo_kernel, peer_allsum_kernel, tags tag0 + it in slot it % 8) against cg_reference.cg:
    stopping iterations on and next to the ring boundaries at 8 and 16, chunks 0, 1 and 3, on a lattice, a band, a
    tridiagonal operator of 257 rows, the operator without neighbours (two ranks) and the band with three neighbours.  The
    ranks' x joined is the solution; return code, iteration count and residual are the same on every rank, and a solve gives
    the same bits with every chunk."""
    per_rank = ranks("coarse", n_ranks)
    worst = {}
    for name in RC.coarse_operators(n_ranks):
        for k in RC.COARSE_KS[name]:
            tol, ref = RC.stop_case(name, k)
            first = None
            for chunk in RC.COARSE_CHUNKS:
                got = coarse_result(per_rank, f"{name}_k{k}_c{chunk}")
                worst[name] = max(worst.get(name, 0.0), coarse_check(got, ref, name, (n_ranks, name, k, chunk)))
                first = first or got
                same_bits(got, first, (n_ranks, name, k, chunk))   # whatever the chunk and whatever ran on the context before
        assert all(int(res[f"{name}_variant"][0]) == 2 for res in per_rank)
    for res in per_rank:
        check_info(res["csr_info"], n_ranks, True, ring="fine-grained")
        check_info(res["comm_info"], n_ranks, True, ring="fine-grained")
    say(f"coarse CG on {n_ranks} ranks", **worst)


@pytest.mark.parametrize("n_ranks", RC.RANKS)
def test_coarse_cg_sequence_on_one_context(ranks, n_ranks):
    """cg_reference.SEQUENCE without reloading: stop 25, 3, 20, a zero right-hand side, stop 9, refused at 5, stop 17.  The tags
    of a solve start coarse_maxit + 16 behind those of the solve before, with max_it 1000 and 5.  A refused solve returns
    GMG_ERR_COARSE_NOCONV on every rank, not GMG_ERR_COMM."""
    per_rank = ranks("coarse", n_ranks)
    worst = 0.0
    for i, (kind, k) in enumerate(R.SEQUENCE):
        got = coarse_result(per_rank, f"seq{i}")
        if kind == "zero":
            assert got[1:] == (0, 0.0, capi().OK) and not got[0].any(), (n_ranks, got[1:])
            continue
        ref = RC.stop_case("csr", k)[1] if kind == "stop" else RC.refused_case("csr", k)[1]
        if kind == "refuse":
            assert ref.status == R.NOCONV and got[3] == capi().ERR_COARSE_NOCONV, (n_ranks, got[1:])
        worst = max(worst, coarse_check(got, ref, "csr", (n_ranks, "sequence", kind, k)))
    say(f"coarse CG sequence on {n_ranks} ranks", x=worst)


# ------------------------------------------------------------------------------------------------ d. outer CG

@pytest.mark.parametrize("pc", ["identity", "jacobi"])
@pytest.mark.parametrize("n_ranks", RC.OUTER_RANKS)
def test_outer_cg_on_a_partitioned_system(ranks, n_ranks, pc):
    """gmg_cg_solve on owned rows of the 13 x 11 x 9 lattice through outer_check of tests/test_gpu_coarse_cg.py: zero and random
    start, a start vector that already meets the tolerance, b = 0, and max_it reached"""
    per_rank = ranks("outer", n_ranks)
    C = capi()
    m = RC.operator("csr")
    norm_b = float(R.cg(m, R.rhs("csr"), np.inf, 0, tier="ld").res)

    def result(what):
        status, it, r0, r = same_on_all(per_rank, f"{pc}_{what}_m")
        return {"status": int(status), "iterations": int(it), "starting_value": float(r0), "convergence_value": float(r),
                "x": joined(per_rank, f"{pc}_{what}_x")}

    worst = 0.0
    for what in ("zero", "random", "max_it"):
        ref = R.stop_case("csr", R.OUTER_K, pc, what)[1] if what != "max_it" else R.refused_case("csr", R.OUTER_MAX_IT, pc)[1]
        r = result(what)
        outer_check(r, ref, ("outer", n_ranks, pc, what))
        worst = max(worst, float(np.abs(r["x"] - ref.x).max() / (R.x_tolerance("csr") * np.abs(ref.x).max())))
    x0, tol, ref = R.converged_start_case(pc)
    r = result("converged")
    assert (r["status"], r["iterations"]) == (C.OK, 0) and np.array_equal(r["x"], x0)
    assert abs(r["starting_value"] - ref.res) <= 1e-12 * norm_b and r["convergence_value"] == r["starting_value"]
    r = result("b0")
    assert (r["status"], r["iterations"], r["starting_value"], r["convergence_value"]) == (C.OK, 0, 0.0, 0.0) and not r["x"].any()
    for res in per_rank:
        check_info(res["info"], n_ranks, False)
    say(f"outer CG ({pc}) on {n_ranks} ranks", x=worst)


# ------------------------------------------------------------------------------------------------ e. smoother and V-cycle

def write_hierarchy(name, directory):
    """the hierarchy, the smoother vectors and the V-cycle sources of tests/mg_cases.py as plain arrays for the ranks"""
    import mg_cases as K

    path = os.path.join(directory, name + ".npz")
    if os.path.exists(path):
        return
    h, H = K.hierarchy(name)
    d = {"n_levels": np.array(len(h.level_matrices))}

    def put(key, m):
        if m is not None and m.nnz > 0:
            d[key + "_rowptr"], d[key + "_col"], d[key + "_val"] = np.asarray(m.rowptr, np.int64), np.asarray(m.col, np.int32), np.asarray(m.val)
            d[key + "_ncols"] = np.array(m.n_cols)

    put("system", h.system_matrix)
    for l in range(len(h.level_matrices)):
        put(f"level{l}", h.level_matrices[l])
        put(f"edge{l}", h.edge_matrices[l])
        d[f"copyg{l}"], d[f"copyl{l}"] = np.asarray(h.copy_global[l], np.int32), np.asarray(h.copy_level[l], np.int32)
        if l > 0:
            d[f"u0_{l}"], d[f"rhs_{l}"] = K.smoother_vectors(name, l)
    for l, P in enumerate(h.prolongations):
        put(f"prol{l}", P)
    d["src"], _, d["dst0"] = K.vcycle_sources(name)
    np.savez(path, **d)


MG_LAUNCHES = [(name, part, n) for name in RC.MG_HIERARCHIES for part in ("part", "repl") for n in RC.MG_RANKS]


@pytest.mark.parametrize("name,part,n_ranks", MG_LAUNCHES)
def test_smoother_step_on_ranks(ranks, name, part, n_ranks):
    """gmg_smoother_step for SSOR on both upper levels of A3 and B3 with level 0 partitioned and replicated: B = 1 and 3 (the
    sweep is split among three ranks, every one of two ranks sweeps everything), B = N and 2 N (one and two blocks per rank)
    and caller-given partitions of N blocks with an empty block and a block of one row (pieces of unequal length, one of
    length zero); 1, 2 and 3 steps, apply and smooth, against mg_cases.smoother_reference with its tolerance.  All ranks return
    the same bits."""
    import mg_cases as K
    import mg_reference as MR

    per_rank = ranks(f"mg-{name}-{part}", n_ranks)
    H = K.hierarchy(name)[1]
    worst = {}
    for key, blocks in RC.block_keys(n_ranks).items():
        for level in range(1, H.n_levels):
            n = H.rows[level]
            bounds = ((level, RC.given_bounds(n_ranks, n)[int(key[5:])]),) if blocks is None else ()
            for steps in RC.MG_STEPS:
                cfg = MR.Config(kind=MR.SSOR, steps=steps, blocks=blocks or n_ranks, bounds=bounds)
                for from_zero in (True, False):
                    got = same_on_all(per_rank, f"sm_{key}_l{level}_s{steps}_z{int(from_zero)}")
                    ref = K.smoother_reference(name, level, cfg, from_zero)
                    err = float(np.linalg.norm(got - ref.ref))
                    worst[key] = max(worst.get(key, 0.0), err / ref.tol)
                    assert err <= ref.tol, (n_ranks, key, level, cfg.label(), from_zero, err, ref.tol)
    say(f"smoother_step {name} ({'partitioned' if part == 'part' else 'replicated'} level 0) on {n_ranks} ranks", **worst)


@pytest.mark.parametrize("name,part,n_ranks", MG_LAUNCHES)
def test_precondition_on_ranks(ranks, name, part, n_ranks):
    """gmg_precondition on owned slices of the sources of mg_cases.vcycle_sources (the dist branches of vcycle: all-gather of the
    source, coarse_level_solve with its all-gather, the split SSOR sweep) with the configurations of mg_cases.VCYCLE_CONFIGS,
    SSOR sweeping one block per rank, through check_vcycle of tests/test_gpu_mg_reference.py with the reference's tolerance and its coarse allowance"""
    import mg_cases as K
    import mg_reference as MR
    from test_gpu_mg_reference import check_vcycle

    per_rank = ranks(f"mg-{name}-{part}", n_ranks)
    H = K.hierarchy(name)[1]
    src = K.vcycle_sources(name)[0]
    worst = {}
    for kind, steps, degree in RC.VCYCLE_CONFIGS:
        cfg = MR.Config(kind=kind, steps=steps, degree=degree, blocks=n_ranks if kind == MR.SSOR and steps > 0 else 1)
        assert cfg in K.VCYCLE_CONFIGS + K.RANK_VCYCLE_CONFIGS
        got = np.stack([joined(per_rank, f"pc_{kind}_{steps}_{j}") for j in range(src.shape[1])], axis=1)
        r = check_vcycle(name, cfg, got, H.cg_allowance(cfg, TAU), (n_ranks, part))
        worst[MR.KIND_NAMES[kind]] = max(worst.get(MR.KIND_NAMES[kind], 0.0), r[0])
    for res in per_rank:
        check_info(res["info"], n_ranks, part == "part")
    say(f"precondition {name} ({'partitioned' if part == 'part' else 'replicated'} level 0) on {n_ranks} ranks", **worst)
