"""The fused kernel's boundary in a rocprofv3 kernel trace (development tool):
per fused grid size and step kind, the fused kernel's duration, the gap from
its end to the start of the finalize that follows (finalize_fast_kernel, or
finalize_slices_kernel + finalize_fast_kernel on a sliced handle), the
finalize kernels' summed duration and the span from the fused kernel's start
to the last finalize kernel's end.

A step is `resample` when the scan kernels launched since the previous fused
launch took at least `--split` x the least such time at that grid (the scan
passes gate on the device's resample flag: their no-op launches are short),
`idle` otherwise.

    python tools/boundary_gaps.py prof/bench_kernel_trace.csv [--split 3] [--fused pf_fused_kernel<1, 1]
"""
import argparse
import collections
import csv

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("trace")
ap.add_argument("--split", type=float, default=3.0)
ap.add_argument("--fused", default="pf_fused_kernel<1, 1, false")   # <motion, lik, host noise, WT>: either store form
args = ap.parse_args()

rows = []
for r in csv.DictReader(open(args.trace)):
    n = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("slam::", "")
    g = int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0)
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n, g))
rows.sort()

recs = collections.defaultdict(list)      # grid -> (scan_us, fused_us, gap_us, first finalize, finalize_us, span_us)
scan = 0.0
for i, (s, e, n, g) in enumerate(rows):
    if "scan" in n:
        scan += (e - s) / 1e3
    if args.fused not in n:
        continue
    j = i + 1
    while j < len(rows) and rows[j][2].startswith("finalize"):
        j += 1
    if j > i + 1:
        fin = rows[i + 1:j]
        recs[g].append((scan, (e - s) / 1e3, (fin[0][0] - e) / 1e3, fin[0][2],
                        sum(f[1] - f[0] for f in fin) / 1e3, (fin[-1][1] - s) / 1e3))
    scan = 0.0


def q(v):
    v = np.asarray(v)
    p = np.percentile(v, [10, 50, 90])
    return f"mean {v.mean():7.2f}  p10 {p[0]:7.2f}  p50 {p[1]:7.2f}  p90 {p[2]:7.2f}"


for g, v in sorted(recs.items()):
    thr = args.split * float(np.percentile([x[0] for x in v], 25))
    nxt = collections.Counter(x[3] for x in v).most_common(1)[0][0]
    print(f"{args.fused} grid={g} ({len(v)} launches; next kernel {nxt}; resample: scans >= {thr:.1f} us)")
    for kind, sel in (("idle", [x for x in v if x[0] < thr and x[3] == nxt]),
                      ("resample", [x for x in v if x[0] >= thr and x[3] == nxt]),
                      ("all", [x for x in v if x[3] == nxt])):
        if not sel:
            continue
        print(f"  {kind:8s} n={len(sel):4d}  scans {np.mean([x[0] for x in sel]):7.2f} us")
        print(f"     fused          {q([x[1] for x in sel])}")
        print(f"     gap            {q([x[2] for x in sel])}")
        print(f"     finalize       {q([x[4] for x in sel])}")
        print(f"     fused start -> finalize end  {q([x[5] for x in sel])}")
