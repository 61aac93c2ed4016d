#!/usr/bin/env python3
"""Does a whole sweep direction fit the LDS as ONE self-contained range?  ("One range per direction".)

Builds the hierarchy of a BASELINE workload after `cycles` adaptive cycles on the CPU (the earlier cycles are solved by
the oracle, as tests/test_ssor_partition.py does) and runs the library's slot allocator (gmg_ssor_slot_plan: host CSR,
no device) on every level >= 1 and every block of the equal-runs partition: steps per direction and the most y slots
live at once, forward and backward, against the capacity of the four-wave sweep -- for the stage-by-stage schedule and for the
rows scheduled by slack (gmg_ssor_slot_plan_packed; DESIGN.md 4, "Rows scheduled by slack"), beside the number of stages,
which is the critical path.

usage: sgs_live_set.py NACL [CYCLES [BLOCKS]]     (NACL: 1 atoms8, 5 atoms1000, 10 atoms8000, 20 atoms64000, 40 stress201)"""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("geometric-multigrid-preconditioners-for-long-range-coulomb-interaction_amd")
from oracle import gmg_oracle as go
S, capi = pkg.step50, pkg.capi
CAPACITY = 12256  # kPhYSlots (gmg_sgs_phase.hpp)
nacl = int(sys.argv[1]); cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 5; blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 1
p = S.Problem(S.prm_text(left=0, right=float(nacl), mesh_size=0.25, vacuum=10, problem="GaussianCharges", dim=3, bc="Inhomogeneous",
                         cycles=cycles, r_c=0.5, cutoff=3.5, rhs_optimization=True, quad_rhs=1, global_refinement=0, smoother="SSOR",
                         refinement_estimator=os.environ.get("STEP50_ESTIMATOR", "Kelly")))
p.set_nacl_atoms(nacl)
for c in range(cycles):
    p.run_cycle(c, on_device=False)
    h = p.hierarchy()
    if c < cycles - 1:
        p.finish_cycle_with(go.OracleMG(h, smoother=go.SSOR).solve(h.system_rhs, x0=p.vector("initial_guess"))["x"])
def depth(A, n, nb):
    """the most dependency stages of a block (the critical path no schedule goes below): stage(i) = 1 + max stage(j) over the
    j < i of the block coupled to i through a stored nonzero a_ij or a_ji"""
    rp, col, val = np.asarray(A.rowptr, np.int64), np.asarray(A.col, np.int64), np.asarray(A.val)
    r = np.repeat(np.arange(n), np.diff(rp))
    out = 0
    for b in range(nb):
        rb, re = n * b // nb, n * (b + 1) // nb
        keep = (r >= rb) & (r < re) & (col >= rb) & (col < re) & (val != 0) & (r != col)
        lo, hi = np.minimum(r[keep], col[keep]) - rb, np.maximum(r[keep], col[keep]) - rb
        order = np.argsort(hi, kind="stable")
        lo, starts = lo[order], np.searchsorted(hi[order], np.arange(re - rb + 1))
        stage = np.zeros(re - rb, np.int64)
        for i in range(re - rb):
            if starts[i + 1] > starts[i]:
                stage[i] = stage[lo[starts[i]:starts[i + 1]]].max() + 1
        out = max(out, int(stage.max()) + 1 if len(lo) else 0)
    return out


print(f"nacl {nacl}, cycle {cycles - 1}, levels {[m.n_rows for m in h.level_matrices]}, {blocks} block(s)")
print("| level | rows | coupled | stages | steps / dir | max live slots, fwd | max live slots, bwd | packed: steps / dir | packed: live fwd | packed: live bwd "
      "| capacity | one range per direction | packed fits |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
for level in range(1, len(h.level_matrices)):
    A = h.level_matrices[level]
    n = A.n_rows
    nb = max(1, min(blocks, (n + 63) // 64))
    coupled = steps = psteps = 0
    live, plive = [0, 0], [0, 0]
    for b in range(nb):
        rb, re = n * b // nb, n * (b + 1) // nb
        for d in (0, 1):
            st, _, _, n_steps, n_slots = capi.ssor_slot_plan(A, rb, re, d)
            live[d] = max(live[d], n_slots)
            if d == 0:
                coupled += int((st >= 0).sum()); steps = max(steps, n_steps)
            # rows scheduled by slack: the same allocator over the packed levels
            _, _, _, n_psteps, n_pslots = capi.ssor_slot_plan(A, rb, re, d, packed=True)
            plive[d] = max(plive[d], n_pslots); psteps = max(psteps, n_psteps)
    fits, pfits = ((max(v) + 1) // 2 * 2 <= CAPACITY for v in (live, plive))
    print(f"| {level} | {n} | {coupled} | {depth(A, n, nb)} | {steps} | {live[0]} | {live[1]} | {psteps} | {plive[0]} | {plive[1]} | {CAPACITY} | "
          f"{'yes' if fits else 'NO: ranged plan'} | {'yes' if pfits else 'NO: stages'} |", flush=True)
