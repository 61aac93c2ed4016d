#!/usr/bin/env python3
"""Per-solve kernel table from a rocprofv3 --kernel-trace (+ --memory-copy-trace) run of bench.py.

  python tools/solve_glue_table.py PROF_DIR [--out TABLE.md] [--title TEXT]

One solve = the window between the first SSOR sweep launch of the second-to-last SSOR solve and the first sweep launch
of the last one: it holds the tail of one solve and the head of the next, i.e. every kernel of one solve exactly once,
whatever the host does between them.  Solves are told apart by the largest gaps between sweep launches.  The gap sum
leaves out the single largest gap of the window (the host between two solve calls)."""
import argparse
import collections
import csv
import glob
import os
import re
import sys

SWEEP = ("sgs_phase_kernel", "sgs_regs_kernel", "sgs_dep_kernel", "sgs_wave_kernel")
COARSE = ("spmv_lattice_kernel", "spmv_sell", "cg_update", "cg_xflush", "cg_direction_kernel", "cg_init")  # (not the outer CG's cg_outer_*)


def short(name):
    name = re.sub(r"^void ", "", name)
    m = re.match(r"([^(]*)", name)
    return (m.group(1) if m else name).strip()[-70:]


def load(d):
    ev = []
    for f in glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    for f in glob.glob(os.path.join(d, "**", "*_memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "memcpy " + r.get("Direction", "?").replace("MEMORY_COPY_", "")))
    ev.sort()
    return ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("prof")
    ap.add_argument("--out", default=None)
    ap.add_argument("--title", default="kernels of one solve")
    ap.add_argument("--solves", type=int, default=4, help="identical solves at the end of the trace (cycle solve + warmup + steps)")
    ap.add_argument("--sweeps-per-solve", type=int, default=None,
                    help="sweep launches of one solve (config.smoothers.*.sweep_launches_per_solve of the bench line); default: found from the gaps")
    a = ap.parse_args()
    ev = load(a.prof)
    sw = [i for i, e in enumerate(ev) if any(s in e[2] for s in SWEEP)]
    if len(sw) < 8:
        sys.exit("no SSOR sweep launches in the trace")
    # sweep launches per solve: the last `solves` solves are identical, so the sequence of sweep launches ends with
    # `solves` equal groups; the groups are separated by the largest gaps between consecutive sweep launches
    gaps = sorted(((ev[sw[k]][0] - ev[sw[k - 1]][1], k) for k in range(1, len(sw))), reverse=True)
    cuts = sorted(k for _, k in gaps[: a.solves + 8])
    per = a.sweeps_per_solve
    for c2 in ([] if per else reversed(cuts)):  # the last cut whose distance to the end repeats once more before it
        n = len(sw) - c2
        if c2 - n in cuts and n >= 8:
            per = n
            break
    if per is None:
        sys.exit("could not tell the solves apart")
    i0, i1 = sw[len(sw) - 2 * per], sw[len(sw) - per]
    win = ev[i0:i1]
    rows = collections.OrderedDict()
    for s, e, n in win:
        c = rows.setdefault(n, [0, 0.0])
        c[0] += 1
        c[1] += (e - s) / 1e3
    g = [max(0, win[k][0] - max(x[1] for x in win[max(0, k - 4):k])) / 1e3 for k in range(1, len(win))]
    g.append(max(0, ev[i1][0] - max(x[1] for x in win[-4:])) / 1e3)
    gmax = max(g)
    span = (ev[i1][0] - ev[i0][0]) / 1e3

    def cls(n):
        if any(s in n for s in SWEEP):
            return "sweep"
        if any(s in n for s in COARSE):
            return "coarse"
        return "glue"

    lines = [f"# {a.title}", "",
             f"One solve of the timed cycle ({per} sweep launches), {span / 1e3:.3f} ms from first sweep launch to first sweep launch.", "",
             "| kernel / copy | class | calls per solve | us per solve | us per call |", "|---|---|---:|---:|---:|"]
    tot = collections.defaultdict(lambda: [0, 0.0])
    for n, (c, us) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
        lines.append(f"| `{n}` | {cls(n)} | {c} | {us:.1f} | {us / c:.2f} |")
        tot[cls(n)][0] += c
        tot[cls(n)][1] += us
    lines += ["", "| class | calls per solve | us per solve |", "|---|---:|---:|"]
    for k in ("sweep", "coarse", "glue"):
        lines.append(f"| {k} | {tot[k][0]} | {tot[k][1]:.1f} |")
    busy = sum(v[1] for v in tot.values())
    lines += ["", f"Sum of the gaps between consecutive kernels: {sum(g) - gmax:.1f} us per solve over {len(g) - 1} gaps "
              f"(the largest gap, {gmax:.1f} us, is the host between two solve calls and is left out); kernels busy {busy:.1f} us."]
    txt = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt)
    sys.stdout.write(txt)


if __name__ == "__main__":
    main()
