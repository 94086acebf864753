"""Duration distribution of selected kernels in a rocprofv3 kernel trace
(development tool): per (kernel, grid) the count and quantiles, split into
the launches below and above `--split` x the fastest one (a device-gated
kernel's no-op launches against its working ones).

    python tools/kdist.py prof/bench_kernel_trace.csv scan_lean finalize [--split 3]

With `--by-prev NAME` every other selected kernel's launches are split instead
by the kind of the latest launch of kernel NAME before them (in start order):
`after low` follows a no-op launch of NAME, `after high` a working one -- the
fused kernel's launches on idle and on resampling steps with NAME = scan_lean.
"""
import argparse
import collections
import csv

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("trace")
ap.add_argument("kernels", nargs="*", help="substrings of the kernel names to keep (all if none)")
ap.add_argument("--split", type=float, default=3.0)
ap.add_argument("--by-prev", default=None, help="substring of the gating kernel's name")
args = ap.parse_args()

d = collections.defaultdict(list)
rows = []
for r in csv.DictReader(open(args.trace)):
    n = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("slam::", "")
    if args.kernels and not any(a in n for a in args.kernels):
        continue
    g = int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0)
    us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000
    d[(n, g)].append(us)
    rows.append((int(r["Start_Timestamp"]), n, g, us))


def q(v):
    v = np.asarray(v)
    if not len(v):
        return "-"
    p = np.percentile(v, [10, 50, 90])
    return f"n={len(v):5d} mean={v.mean():8.2f} p10={p[0]:8.2f} p50={p[1]:8.2f} p90={p[2]:8.2f}"


for (k, g), v in sorted(d.items()):
    v = np.asarray(v)
    lo = v[v < args.split * v.min()]
    hi = v[v >= args.split * v.min()]
    print(f"{k} grid={g}\n   low : {q(lo)}\n   high: {q(hi)}")

if args.by_prev:
    gate = [us for _, n, _, us in rows if args.by_prev in n]
    if not gate:
        raise SystemExit(f"no launch of a kernel matching {args.by_prev!r} among the selected ones")
    thr = args.split * min(gate)
    after = collections.defaultdict(lambda: ([], []))
    kind = None
    for _, n, g, us in sorted(rows):
        if args.by_prev in n:
            kind = us >= thr
        elif kind is not None:
            after[(n, g)][kind].append(us)
    print(f"--- split by the latest {args.by_prev} launch before (working: >= {thr:.2f} us)")
    for (k, g), (lo, hi) in sorted(after.items()):
        print(f"{k} grid={g}\n   after low : {q(lo)}\n   after high: {q(hi)}")
