#!/usr/bin/env python3
"""One rank of tests/test_gpu_ranks_reference.py and tests/test_gpu_ranks_layouts.py: opens a context on the communicator named
by the id, runs the steps of one group of tests/rank_cases.py and writes everything it computed to one .npz (arrays, iteration
counts, residuals, return codes, the debug_upload lines of an upload, comm_info()).  It judges nothing: the parent compares with the references.  numpy and the library only.

usage: rank_worker.py RANK N_RANKS ID_HEX GROUP OUT_NPZ
(the smoother groups read their hierarchy and vectors from <directory of OUT_NPZ>/<hierarchy>.npz, written by the parent)"""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # repo root: the package
import cg_reference as R  # noqa: E402
import partition_reference as PR  # noqa: E402
import rank_cases as RC  # noqa: E402
from gpu_util import capi  # noqa: E402

TAU = 1e-10


def set_local(c, which, set_matrix, m, rank, n_ranks):
    loc = PR.localize(m, rank, n_ranks)
    set_matrix(loc)
    c.set_halo_plan(which, loc.neighbor_rank, loc.send_count, loc.send_idx, loc.recv_count)
    return loc


def load_partitioned(c, h, rank, n_ranks, partition_level0):
    """What the host driver does for one rank (upload() in csrc/host/laplace_problem.cc), from plain arrays: the global sizes;
    the system matrix, and level 0 when it is partitioned, as owned rows with their halo plans; everything else whole; then
    the ranks meet on the host before the first solve.  h: any object with the attribute names of a hierarchy (system_matrix
    may be None; level_matrices[0] may be None when only the system matrix is used)."""
    n_sys = h.system_matrix.n_rows if h.system_matrix is not None else h.level_matrices[0].n_rows
    n0 = h.level_matrices[0].n_rows if h.level_matrices and h.level_matrices[0] is not None else 0
    c.set_global_sizes(n_sys, n0 if partition_level0 else 0)
    out = SimpleNamespace(system=None, level0=None)
    if h.system_matrix is not None:
        out.system = set_local(c, RC.SYSTEM, c.set_system_matrix, h.system_matrix, rank, n_ranks)
    for l, A in enumerate(h.level_matrices):
        if A is None:
            continue
        if l == 0 and partition_level0:
            out.level0 = set_local(c, 0, lambda loc: c.set_level_matrix(0, loc), A, rank, n_ranks)
        else:
            c.set_level_matrix(l, A)
        I = h.edge_matrices[l] if h.edge_matrices else None
        if I is not None and I.nnz > 0:
            c.set_edge_matrix(l, I)
        if h.copy_global:
            c.set_copy_indices(l, h.copy_global[l], h.copy_level[l])
    for l, P in enumerate(h.prolongations or []):
        c.set_prolongation(l, P)
    c.comm_barrier()
    return out


def one_operator(m, system=True, level0=True):
    return SimpleNamespace(system_matrix=m if system else None, level_matrices=[m if level0 else None], edge_matrices=None,
                           copy_global=None, copy_level=None, prolongations=None)


def vec(c, data):
    """a device vector of the data; one unused entry stands in for an empty slice"""
    data = np.asarray(data, dtype=np.float64)
    return c.vector(max(len(data), 1), data if len(data) else np.array([-7.0]))


def apply(c, fn, *inputs, n_out):
    """fn(out, *device vectors of inputs) -> out[:n_out]"""
    vs = [vec(c, a) for a in inputs]
    vo = vec(c, np.full(max(n_out, 1), np.nan))
    fn(vo, *vs)
    out = vo.download()[:n_out]
    for v in vs + [vo]:
        v.free()
    return out


# ------------------------------------------------------------------------------------------------ groups

def run_collectives(c, rank, N, res):
    tag = 0
    for li, sizes in enumerate(RC.allgather_rounds(N)):
        pairs = []
        for n in sizes:
            b, e = PR.owned_range(n, rank, N)
            pairs.append((n, vec(c, RC.allgather_values(tag, n)[b:e]), vec(c, np.full(N * PR.chunk(n, N), -1.0))))
            tag += 1
        c.comm_barrier()
        for n, src, dst in pairs:           # back to back: nothing waits for the stream in between
            c.allgather(n, dst, src)
        for j, (n, src, dst) in enumerate(pairs):
            res[f"ag{li}_{j}"] = dst.download()[:n]
            src.free(); dst.free()
    for length in RC.REDUCE_LENGTHS:
        x, y = RC.reduce_vectors(length, rank)
        vx, vy = vec(c, x), vec(c, y)
        res[f"dot{length}"] = np.array([c.dot(vx, vy), c.dot(vx, vx)])
        res[f"norms{length}"] = np.array(c.norms(vx))
        vx.free(); vy.free()
    # 20 collectives of four kinds on one context
    m = RC.operator(RC.MIX_OPERATOR)
    n = m.n_rows
    loc = load_partitioned(c, one_operator(m, level0=False), rank, N, False).system
    b, e = loc.row_begin, loc.row_begin + loc.n_rows
    for i, op in enumerate(RC.MIX_OPS):
        x = RC.mix_vector(i, n)[b:e]
        if op == "halo":
            res[f"mix{i}"] = apply(c, lambda out, v: c.spmv(RC.SYSTEM, out, v), x, n_out=e - b)
        elif op == "dot":
            vx, vy = vec(c, x), vec(c, RC.mix_vector(100 + i, n)[b:e])
            res[f"mix{i}"] = np.array([c.dot(vx, vy)])
            vx.free(); vy.free()
        elif op == "allgather":
            g = RC.MIX_GATHER
            gb, ge = PR.owned_range(g, rank, N)
            res[f"mix{i}"] = apply(c, lambda out, v: c.allgather(g, out, v), RC.allgather_values(1000 + i, g)[gb:ge],
                                   n_out=N * PR.chunk(g, N))[:g]
        else:
            vx = vec(c, x)
            res[f"mix{i}"] = np.array(c.norms(vx))
            vx.free()


def run_spmv(c, rank, N, res):
    for name in RC.spmv_operators(N):
        m = RC.operator(name)
        locs = load_partitioned(c, one_operator(m), rank, N, True)
        loc = locs.system
        res[f"{name}_plan"] = np.concatenate([loc.neighbor_rank, loc.send_count, loc.recv_count]).astype(np.int64)
        b, e = loc.row_begin, loc.row_begin + loc.n_rows
        X = RC.spmv_vectors(name)
        for i in range(RC.N_SPMV_VECTORS):
            res[f"{name}_sys{i}"] = apply(c, lambda out, v: c.spmv(RC.SYSTEM, out, v), X[i, b:e], n_out=e - b)
            res[f"{name}_lv{i}"] = apply(c, lambda out, v: c.spmv(0, out, v), X[i, b:e], n_out=e - b)
        # the rounds that follow: a rank without neighbours must still be in step
        x, y = RC.reduce_vectors(257, rank)
        vx, vy = vec(c, x), vec(c, y)
        res[f"{name}_dot"] = np.array([c.dot(vx, vy)])
        vx.free(); vy.free()


def coarse(c, b_local, tol, max_it, chunk):
    c.set_tuning(coarse_chunk=chunk, cg_variant=0)
    c.set_coarse(tol, max_it)
    vb, vx = vec(c, b_local), vec(c, np.full(len(b_local), np.nan))
    it, res, rc = c.coarse_solve(vx, vb)
    x = vx.download()
    vb.free(); vx.free()
    return x, np.array([it, res, rc], dtype=np.float64)


def run_coarse(c, rank, N, res):
    names = RC.coarse_operators(N)
    tols = {(name, k): RC.stop_case(name, k)[0] for name in names for k in RC.COARSE_KS[name]}    # host work first
    tols.update({("csr", k): RC.stop_case("csr", k)[0] for kind, k in R.SEQUENCE if kind == "stop"})
    for name in names:
        m = RC.operator(name)
        loc = load_partitioned(c, one_operator(m, system=False), rank, N, True).level0
        b = RC.rhs(name)[loc.row_begin:loc.row_begin + loc.n_rows]
        for k in RC.COARSE_KS[name]:
            for chunk in RC.COARSE_CHUNKS:
                res[f"{name}_k{k}_c{chunk}_x"], res[f"{name}_k{k}_c{chunk}_m"] = coarse(c, b, tols[name, k], 1000, chunk)
        if name == "csr":   # the sequence on the context as it stands: nothing is reloaded
            for i, (kind, k) in enumerate(R.SEQUENCE):
                if kind == "stop":
                    got = coarse(c, b, tols["csr", k], 1000, 0)
                elif kind == "refuse":
                    got = coarse(c, b, R.REFUSE_TOL, k, 0)
                else:
                    got = coarse(c, np.zeros(len(b)), 1e-10, 1000, 0)
                res[f"seq{i}_x"], res[f"seq{i}_m"] = got
            res["csr_info"] = np.array(json.dumps(c.comm_info()))
        res[f"{name}_variant"] = np.array([int(c.stats().coarse_variant)])


def run_outer(c, rank, N, res):
    C = capi()
    m = RC.operator("csr")
    n = m.n_rows
    loc = load_partitioned(c, one_operator(m, level0=False), rank, N, False).system
    lo, hi = loc.row_begin, loc.row_begin + loc.n_rows
    b = R.rhs("csr")
    norm_b = float(R.cg(m, b, np.inf, 0, tier="ld").res)
    plan = []
    for pc, what in RC.OUTER_CASES:     # host work first
        if what in ("zero", "random"):
            tol = R.stop_case("csr", R.OUTER_K, pc, what)[0]
            plan.append((pc, what, b, R.x_start("csr") if what == "random" else np.zeros(n), tol / norm_b, 500))
        elif what == "converged":
            x0, tol, _ = R.converged_start_case(pc)
            plan.append((pc, what, b, x0, tol / norm_b, 500))
        elif what == "b0":
            plan.append((pc, what, np.zeros(n), np.zeros(n), 1e-8, 500))
        else:
            plan.append((pc, what, b, np.zeros(n), R.REFUSE_TOL / norm_b, R.OUTER_MAX_IT))
    c.comm_barrier()
    for pc, what, rhs, x0, rel_tol, max_it in plan:
        vb, vx = vec(c, rhs[lo:hi]), vec(c, x0[lo:hi])
        r = c.cg_solve(vx, vb, rel_tol=rel_tol, max_it=max_it, precond={"identity": C.PRECOND_IDENTITY, "jacobi": C.PRECOND_JACOBI}[pc])
        res[f"{pc}_{what}_x"] = vx.download()
        res[f"{pc}_{what}_m"] = np.array([r["status"], r["iterations"], r["starting_value"], r["convergence_value"]], dtype=np.float64)
        vb.free(); vx.free()
    res["info"] = np.array(json.dumps(c.comm_info()))


def captured(fn, path):
    """what fn() writes to the process's standard error (the library's debug_upload lines), kept in the rank's log as well"""
    sys.stderr.flush()
    saved, fd = os.dup(2), os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
    os.dup2(fd, 2)
    try:
        fn()
    finally:
        os.dup2(saved, 2)
        os.close(saved)
        os.close(fd)
    with open(path) as f:
        text = f.read()
    os.unlink(path)
    sys.stderr.write(text)
    return text


def load_layout(c, m, rank, N, system, level0, log_path):
    """load_partitioned for one operator with debug_upload on: (owned rows, log of the system matrix's upload, log of level 0's)"""
    c.set_global_sizes(m.n_rows, m.n_rows if level0 else 0)
    c.set_option("debug_upload", 1)
    logs, locs = {}, []
    if system:
        logs["sys"] = captured(lambda: locs.append(set_local(c, RC.SYSTEM, c.set_system_matrix, m, rank, N)), log_path)
    if level0:
        logs["lv"] = captured(lambda: locs.append(set_local(c, 0, lambda l: c.set_level_matrix(0, l), m, rank, N)), log_path)
    c.set_option("debug_upload", 0)
    c.comm_barrier()
    return locs[0], logs


def run_layout_spmv(c, rank, N, res, log_path):
    """every operator of RC.LAYOUT_OPERATORS as system matrix and as partitioned level 0, under each of its option sets"""
    for name in RC.LAYOUT_OPERATORS:
        m = RC.operator(name)
        X = RC.spmv_vectors(name)
        loc = None
        for variant, options in RC.LAYOUT_VARIANTS[name]:
            for key, value in options.items():
                c.set_option(key, value)
            if loc is None or any(key in RC.UPLOAD_OPTIONS for key in options):
                loc, logs = load_layout(c, m, rank, N, True, True, log_path)
                res[f"{name}_{variant}_syslog"], res[f"{name}_{variant}_lvlog"] = np.array(logs["sys"]), np.array(logs["lv"])
                res[f"{name}_{variant}_layout"] = np.array([int(c.stats().spmv0_layout)])
            b, e = loc.row_begin, loc.row_begin + loc.n_rows
            for i in range(RC.N_SPMV_VECTORS):
                res[f"{name}_{variant}_sys{i}"] = apply(c, lambda out, v: c.spmv(RC.SYSTEM, out, v), X[i, b:e], n_out=e - b)
                res[f"{name}_{variant}_lv{i}"] = apply(c, lambda out, v: c.spmv(0, out, v), X[i, b:e], n_out=e - b)
            for key in options:
                c.set_option(key, 0)
        x, y = RC.reduce_vectors(257, rank)
        vx, vy = vec(c, x), vec(c, y)
        res[f"{name}_dot"] = np.array([c.dot(vx, vy)])
        vx.free(); vy.free()


def run_layout_coarse(c, rank, N, res, log_path):
    names = RC.layout_coarse_operators(N)
    tols = {(name, k): RC.stop_case(name, k)[0] for name in names for k in RC.LAYOUT_COARSE_KS[name]}    # host work first
    for name in names:
        m = RC.operator(name)
        loc, logs = load_layout(c, m, rank, N, False, True, log_path)
        res[f"{name}_lvlog"], res[f"{name}_layout"] = np.array(logs["lv"]), np.array([int(c.stats().spmv0_layout)])
        b = RC.rhs(name)[loc.row_begin:loc.row_begin + loc.n_rows]
        for k in RC.LAYOUT_COARSE_KS[name]:
            for chunk in RC.COARSE_CHUNKS:
                res[f"{name}_k{k}_c{chunk}_x"], res[f"{name}_k{k}_c{chunk}_m"] = coarse(c, b, tols[name, k], 1000, chunk)
        res[f"{name}_variant"] = np.array([int(c.stats().coarse_variant)])
        res[f"{name}_info"] = np.array(json.dumps(c.comm_info()))


def run_layout_outer(c, rank, N, res, log_path):
    C = capi()
    name = RC.LAYOUT_OUTER
    m = RC.operator(name)
    n = m.n_rows
    b = RC.rhs(name)
    norm_b = float(R.cg(m, b, np.inf, 0, tier="ld").res)
    plan = []
    for pc, what in RC.LAYOUT_OUTER_CASES:     # host work first
        if what in ("zero", "random"):
            plan.append((pc, what, b, RC.x_start(name) if what == "random" else np.zeros(n), RC.outer_case(name, pc, what)[0] / norm_b, 500))
        elif what == "b0":
            plan.append((pc, what, np.zeros(n), np.zeros(n), 1e-8, 500))
        else:
            plan.append((pc, what, b, np.zeros(n), R.REFUSE_TOL / norm_b, R.OUTER_MAX_IT))
    loc, logs = load_layout(c, m, rank, N, True, False, log_path)
    res["syslog"] = np.array(logs["sys"])
    lo, hi = loc.row_begin, loc.row_begin + loc.n_rows
    for pc, what, rhs, x0, rel_tol, max_it in plan:
        vb, vx = vec(c, rhs[lo:hi]), vec(c, x0[lo:hi])
        r = c.cg_solve(vx, vb, rel_tol=rel_tol, max_it=max_it, precond={"identity": C.PRECOND_IDENTITY, "jacobi": C.PRECOND_JACOBI}[pc])
        res[f"{pc}_{what}_x"] = vx.download()
        res[f"{pc}_{what}_m"] = np.array([r["status"], r["iterations"], r["starting_value"], r["convergence_value"]], dtype=np.float64)
        vb.free(); vx.free()
    res["info"] = np.array(json.dumps(c.comm_info()))


def read_hierarchy(path):
    z = np.load(path)

    def csr(key):
        if key + "_rowptr" not in z:
            return None
        rp, col, val = z[key + "_rowptr"], z[key + "_col"], z[key + "_val"]
        return SimpleNamespace(n_rows=len(rp) - 1, n_cols=int(z[key + "_ncols"]), rowptr=rp, col=col, val=val, nnz=len(col))

    L = int(z["n_levels"])
    h = SimpleNamespace(system_matrix=csr("system"), level_matrices=[csr(f"level{l}") for l in range(L)],
                        edge_matrices=[csr(f"edge{l}") for l in range(L)], prolongations=[csr(f"prol{l}") for l in range(L - 1)],
                        copy_global=[z[f"copyg{l}"] for l in range(L)], copy_level=[z[f"copyl{l}"] for l in range(L)])
    return h, z


def run_mg(c, rank, N, res, name, partitioned, directory):
    h, z = read_hierarchy(os.path.join(directory, name + ".npz"))
    L = len(h.level_matrices)
    n_sys = h.system_matrix.n_rows
    for key, blocks in RC.block_keys(N).items():
        c.set_tuning(ssor_blocks=blocks if blocks else N)
        for level in range(1, L):
            n = h.level_matrices[level].n_rows
            c.set_ssor_block_rows(level, RC.given_bounds(N, n)[int(key[5:])] if blocks is None else [])
        loc = load_partitioned(c, h, rank, N, partitioned).system
        for level in range(1, L):
            u0, rhs = z[f"u0_{level}"], z[f"rhs_{level}"]
            for steps in RC.MG_STEPS:
                c.set_smoother(RC.SSOR, 0.5, steps)
                for from_zero in (True, False):
                    res[f"sm_{key}_l{level}_s{steps}_z{int(from_zero)}"] = apply(
                        c, lambda out, u, r: (c.equ(out, 1.0, u), c.smoother_step(level, out, r, from_zero)), u0, rhs, n_out=len(u0))
        if key == f"B{N}":
            src, dst0 = z["src"], z["dst0"]
            lo, hi = loc.row_begin, loc.row_begin + loc.n_rows
            c.set_coarse(TAU, 1000)
            for kind, steps, degree in RC.VCYCLE_CONFIGS:
                c.set_smoother(kind, 0.5, steps, cheb_degree=degree, cheb_ratio=30.0, cheb_lmax=0.0)
                for j in range(src.shape[1]):
                    vs, vd = vec(c, src[lo:hi, j]), vec(c, dst0[lo:hi])
                    c.precondition(vd, vs)
                    res[f"pc_{kind}_{steps}_{j}"] = vd.download()[:hi - lo]
                    vs.free(); vd.free()
            res["info"] = np.array(json.dumps(c.comm_info()))


def main():
    rank, N, uid, group, out = int(sys.argv[1]), int(sys.argv[2]), bytes.fromhex(sys.argv[3]), sys.argv[4], sys.argv[5]
    n_levels = 1
    if group.startswith("mg-"):
        _, name, part = group.split("-")
        n_levels = int(np.load(os.path.join(os.path.dirname(out), name + ".npz"))["n_levels"])
    c = capi().Context(n_levels)
    c.comm_init(rank, N, uid)
    res = {}
    if group == "collectives":
        run_collectives(c, rank, N, res)
    elif group == "spmv":
        run_spmv(c, rank, N, res)
    elif group == "coarse":
        run_coarse(c, rank, N, res)
    elif group == "outer":
        run_outer(c, rank, N, res)
    elif group.startswith("layout_"):
        {"layout_spmv": run_layout_spmv, "layout_coarse": run_layout_coarse, "layout_outer": run_layout_outer}[group](c, rank, N, res, out + ".upload.txt")
    else:
        run_mg(c, rank, N, res, name, part == "part", os.path.dirname(out))
    res["comm_info"] = np.array(json.dumps(c.comm_info()))
    c.close()
    tmp = out + ".tmp.npz"
    np.savez(tmp, **res)
    os.replace(tmp, out)


if __name__ == "__main__":
    main()
