#!/usr/bin/env python3
"""The default of p_new (slamhip.fastslam.P_NEW_DEFAULT): a sweep of the
float64 oracle (tests/fastslam_da_ref.py, CPU only) on the world of
fast_slam.py's docstring example -- 7 landmarks, a 9 m scan sensor, 4096
particles, 100 steps of the reference's circle.  For each p_new the landmark
count of the final best particle against the number of landmarks the sensor
truly observed; the default is the value whose count is closest (the largest
such value on a tie: the least eager to merge).  DESIGN 11c records the table.

    python tools/fastslam_pnew_sweep.py [--seeds 3]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("slam-robot_simu_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import fastslam_da_ref as da  # noqa: E402
import fastslam_ref as fr  # noqa: E402

NOISE = (0.1, np.deg2rad(3.0), np.deg2rad(3.0))      # ScanSensor's defaults

P_NEW = (1e-6, 1e-4, 1e-3, 1e-2, 3e-2, 0.1, 0.3, 1.0, 3.0)


def world(seed, steps=100):
    """The docstring example's world; the scans by fastslam_ref.observe, the
    CPU restatement of ScanSensor's noise model (ScanSensor itself runs on the
    device)."""
    lm = np.random.RandomState(3).uniform(-12, 12, (7, 2))
    rs = np.random.RandomState(seed)
    pose = np.array([10.0, 0.0, np.pi / 2])
    v, w, dt = 10.0 * np.deg2rad(10.0), np.deg2rad(10.0), 0.1
    scans, seen = [], set()
    for _ in range(steps):
        pose = pose + np.array([v * dt * np.cos(pose[2]), v * dt * np.sin(pose[2]), w * dt])
        ids, obs = fr.observe(pose, lm, 9.0, NOISE, rs)
        seen |= set(ids.tolist())
        scans.append(obs)
    return (v, w), scans, len(seen), lm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--particles", type=int, default=4096)
    a = ap.parse_args()
    n, cap = a.particles, 32
    q = np.diag([0.03, 0.03, np.deg2rad(2.0)]) ** 2
    noise = NOISE
    print(f"# oracle float64, NP {n}, capacity {cap}, 100 steps, ESS_TH NP/2")
    print("# p_new  |  per seed: best particle's count / landmarks observed (worst map error, m)")
    for pn in P_NEW:
        cells, miss = [], 0
        for seed in range(a.seeds):
            ctl, scans, n_obs, lm = world(seed)
            ref = da.FSDARef(n, cap, p_new=pn, noise=noise, ess_th=n / 2.0)
            rs = np.random.RandomState(100 + seed)
            for obs in scans:
                out = ref.step(ctl, obs, rs.multivariate_normal([0.0, 0.0, 0.0], q, n), rs.rand() / n)
            i = out["max_idx"]
            c = int(ref.cnt[i])
            m = ref.mean[i, :c].astype(np.float64)
            err = float(np.max(np.min(np.hypot(m[:, None, 0] - lm[None, :, 0],
                                               m[:, None, 1] - lm[None, :, 1]), axis=1))) if c else 0.0
            miss += abs(c - n_obs)
            cells.append(f"{c}/{n_obs} ({err:.2f})")
        print(f"{pn:8.0e} |  {'   '.join(cells)}   | total |count - observed| = {miss}")


if __name__ == "__main__":
    main()
