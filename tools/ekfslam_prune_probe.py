"""The evidence kernel and the in-place compaction of an associating EKF-SLAM
handle at capacity 10,000 (n = 30,003, P = 7.2 GB) with 100, 1,000 and 10,000
landmarks held.  Writes profiles/ekfslam_prune_ab.txt.

    python tools/ekfslam_prune_probe.py [--reps 5] [--out profiles/ekfslam_prune_ab.txt]

Three cases per count, device time from slam_ekfslam_prune_info, median of
``reps`` after one warm-up, each from a freshly placed state: the evidence
kernel alone (an empty scan that removes nothing), the removal of the last two
slots (only the tail is zeroed), the removal of slot 0 (the whole triangle
moves).  Each compaction is set against a plain device-to-device copy of 2 GB
measured in the same process: ``ideal`` is the time that copy rate needs for the
region's own bytes -- every surviving element at or beyond the first removed
slot read once and written once, the vacated rows written once -- and ``model``
the time it needs for the bytes the three launches move (the column pass reads
and writes the region's columns once more)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-robot_simu_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

CAP = 10000


def traffic(first, count_new, count_old):
    """(ideal bytes, bytes of the three launches) of a compaction."""
    r, n_new, n_old = 3 + 3 * first, 3 + 3 * count_new, 3 + 3 * count_old
    w = np.arange(r, n_new, dtype=np.float64)
    rows = float((w + 1).sum())                 # the moved rows, columns 0 .. w
    cols = float((w - r + 1).sum())             # their columns at or beyond r
    zero = float(n_old - n_new) * n_old
    return 8 * (2 * rows + zero), 8 * (2 * rows + 2 * cols + zero)


def copy_rate():
    """Bytes read plus bytes written per second of a plain 2 GB device copy."""
    import torch
    a = torch.zeros(1 << 28, dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    ms = []
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return 2 * 8 * (1 << 28) / (np.median(ms[1:]) * 1e-3)


def fmt(v):
    v = np.asarray(v) * 1e3
    return f"{np.median(v):10.1f} [{v.min():.1f} .. {v.max():.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ekfslam_prune_ab.txt"))
    args = ap.parse_args()
    from slamhip.ekf import DeviceEKFSLAM
    rate = copy_rate()
    n = 3 + 3 * CAP
    lines = [f"slam_ekfslam evidence pass and compaction, capacity {CAP} (n = {n}); device time in "
             f"us, median of {args.reps} [min .. max]",
             f"plain device-to-device copy of 2 GB: {rate / 1e9:.0f} GB/s (read + written)", ""]
    rs = np.random.RandomState(5)
    d = DeviceEKFSLAM(CAP, association="ml", prune=dict(view_range=1.0, ev_max=100))
    try:
        for count in (100, 1000, 10000):
            na = 3 + 3 * count
            mu, diag = np.zeros(n), np.zeros(n)
            mu[:3], diag[:3] = (0.0, 0.0, 0.7), (1e-4, 1e-4, 1e-5)
            mu[3:na] = np.column_stack([rs.uniform(-200, 200, (count, 2)),
                                        rs.uniform(-3, 3, count)]).ravel()
            diag[3:na] = 0.01
            ev_ms = []
            cases = {"last two slots": [count - 2, count - 1], "slot 0": [0]}
            comp = {q: [] for q in cases}
            mask = {q: [] for q in cases}
            for rep in range(args.reps + 1):
                d.init_diag(mu, diag)
                d.set_count(count)
                d.set_evidence(np.full(CAP, 50))
                d.observe(np.empty((0, 3)))
                info = d.prune_info()
                assert info["removed"] == 0 and info["count_before"] == count
                if rep:
                    ev_ms.append(info["evidence_ms"])
                for q, gone in cases.items():
                    d.init_diag(mu, diag)
                    d.set_count(count)
                    d.remove(gone)
                    info = d.prune_info()
                    assert info["removed"] == len(gone) and d.count == count - len(gone)
                    if rep:
                        comp[q].append(info["compact_ms"])
                        mask[q].append(info["evidence_ms"])
            lines += [f"count = {count} (n_act = {na})",
                      f"  evidence kernel, empty scan, nothing removed   {fmt(ev_ms)}"]
            for q, gone in cases.items():
                ideal, model = traffic(gone[0], count - len(gone), count)
                t = float(np.median(comp[q])) * 1e-3
                lines += [f"  remove {q}: mask kernel {fmt(mask[q])}",
                          f"    compaction {fmt(comp[q])}; region {ideal / 1e6:.2f} MB, launches move "
                          f"{model / 1e6:.2f} MB",
                          f"    at the copy rate: ideal {ideal / rate * 1e6:.1f} us ({ideal / rate / t:.3f} "
                          f"of it achieved), model {model / rate * 1e6:.1f} us ({model / rate / t:.3f})"]
            lines.append("")
    finally:
        d.close()
    text = "\n".join(lines)
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
