#!/usr/bin/env python3
"""What landmark removal buys: tools/fastslam_pnew_sweep.py's world and seeds
(7 landmarks, a 9 m scan sensor, 100 steps of the reference's circle) run on the
float64 oracle (tests/fastslam_da_ref.py, CPU only) with and without the
evidence pass of tests/fastslam_prune_ref.py -- counters +1 / -1, removal below
0, a view range of 7.2 m.  Per p_new: the sum over the seeds of |the best
particle's count - the landmarks the sensor truly observed|, the maps that end
at capacity and the observations dropped.  DESIGN 11f records the table.

    python tools/fastslam_prune_sweep.py [--particles 4096] [--seeds 3] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("slam-robot_simu_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

import fastslam_da_ref as da  # noqa: E402
import fastslam_prune_ref as pr  # noqa: E402
from fastslam_pnew_sweep import NOISE, world  # noqa: E402

P_NEW = (1e-4, 1e-2, 3e-2, 0.1, 0.3)
CAP = 32
VIEW_RANGE = 7.2            # somewhat inside the 9 m sensor


def prune_config():
    return pr.PruneConfig(VIEW_RANGE, init=1, hit=1, miss=1, remove_below=0)


def run(n, p_new, seed, cfg=None):
    """One filter run: (|count - observed| of the final best particle, its
    count, the landmarks observed, observations dropped, particles at capacity,
    landmarks removed)."""
    ctl, scans, n_obs, _ = world(seed)
    q = np.diag([0.03, 0.03, np.deg2rad(2.0)]) ** 2
    ref = da.FSDARef(n, CAP, p_new=p_new, noise=NOISE, ess_th=n / 2.0)
    flt = pr.PruneRef(ref, cfg) if cfg is not None else ref
    rs = np.random.RandomState(100 + seed)
    dropped = removed = 0
    for obs in scans:
        out = flt.step(ctl, obs, rs.multivariate_normal([0.0, 0.0, 0.0], q, n), rs.rand() / n)
        dropped += int((out["assoc"] == da.DROPPED).sum())
        removed += int(out["removed"].sum()) if cfg is not None else 0
    c = int(ref.cnt[out["max_idx"]])
    return dict(miss=abs(c - n_obs), count=c, observed=n_obs, dropped=dropped,
                full=int((ref.cnt == CAP).sum()), removed=removed)


def table(n, seeds, p_news=P_NEW, emit=print):
    emit(f"# oracle float64, NP {n}, capacity {CAP}, 100 steps, ESS_TH NP/2; evidence +1 / -1, "
         f"removal below 0, view range {VIEW_RANGE} m")
    emit("# p_new | without: sum |count - observed| (counts; dropped; particles at capacity) | with: "
         "the same (removed)")
    rows = {}
    for pn in p_news:
        a = [run(n, pn, s) for s in range(seeds)]
        b = [run(n, pn, s, prune_config()) for s in range(seeds)]
        rows[pn] = (a, b)

        def cell(rs_):
            return (f"{sum(r['miss'] for r in rs_):3d} ("
                    f"{' '.join(str(r['count']) + '/' + str(r['observed']) for r in rs_)}; "
                    f"{sum(r['dropped'] for r in rs_)} dropped; "
                    f"{sum(r['full'] for r in rs_)} full")
        emit(f"{pn:8.0e} | {cell(a)}) | {cell(b)}; {sum(r['removed'] for r in b)} removed)")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--particles", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastslam_prune_sweep.txt"))
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    table(a.particles, a.seeds, emit=emit)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
