"""Times the direct coarse solver on cubic level-0 lattices: one coarse solve and each of its passes,
beside the coarse CG on the same right-hand side.

    python tools/coarse_direct_probe.py [--sizes 45 121 201] [--reps 20] [--out FILE.json]

The passes are timed with HIP events attached to their launches (gmg_coarse_direct_profile: the kernels' own begin-to-end
times, median of `reps` solves); `direct_kernels_ms` is their sum.  `direct_solve_ms` and `cg_solve_ms` are host wall time
per solve between two synchronisations of the stream, launch gaps and call overhead included: upper bounds.  The rate of a
pass is 16 bytes per interior vertex (one read, one write) over its kernel time, to be held against
`measured_stream_copy_GBps` of bench.py.  Prints one JSON line per size."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fastdiag_reference as F  # noqa: E402
from gpu_util import capi  # noqa: E402


def timed(c, reps, call):
    call()
    c.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    c.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def probe(nv, reps):
    C = capi()
    shape = (nv, nv, nv)
    n = nv ** 3
    b = F.rhs(shape)
    c = C.Context(1)
    c.set_level_matrix_lattice(0, shape, F.cell_matrix())
    vb, vx, vt = c.vector(n, b), c.vector(n), c.vector(n)
    it_cg, res_cg, rc = c.coarse_solve(vx, vb)
    cg_ms = timed(c, max(1, reps // 10), lambda: c.coarse_solve(vx, vb, False))
    c.set_coarse_solver(C.COARSE_DIRECT)
    it, res, rc = c.coarse_solve(vx, vb)
    out = {"nv": nv, "rows": n, "cg_iterations": it_cg, "cg_residual": res_cg, "cg_solve_ms": cg_ms, "direct_residual": res,
           "direct_solve_ms": timed(c, reps, lambda: c.coarse_solve(vx, vb, False))}
    interior_bytes = 16.0 * (nv - 2) ** 3
    ms = np.median(np.array([c.coarse_direct_profile(vx, vb) for _ in range(reps)]), axis=0)
    out["direct_kernels_ms"] = float(ms.sum())
    for k, name in enumerate(("x", "y", "z_scale", "z_back", "y_back", "x_back")):
        out[f"pass_{name}_ms"] = float(ms[k])
        out[f"pass_{name}_GBps"] = interior_bytes / (ms[k] * 1e-3) / 1e9
    out["boundary_rows_ms"] = float(ms[6])
    rd, cp = c.calibrate_hbm(1 << 28, 5)
    out["stream_copy_GBps"] = cp
    for v in (vb, vx, vt):
        v.free()
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[45, 121, 201])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [json.dumps(probe(nv, a.reps)) for nv in a.sizes]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
