"""The four phases of slam_ekfslam_observe at capacity 10,000 (n = 30,003,
P = 7.2 GB) with k = 20 observations and 100, 1,000 and 10,000 landmarks held,
against a known-id handle of 10,000 landmarks given the same matches (DESIGN
11g).  Writes profiles/ekfslam_assoc_ab.txt.

    python tools/ekfslam_assoc_probe.py [--reps 5] [--out profiles/ekfslam_assoc_ab.txt]

The world: landmarks on a 4 m grid, jittered, the prior 5 cm off with a
diagonal covariance; the handle holds the ``count`` landmarks nearest the robot.
A scan is the 18 nearest landmarks and two sightings far beyond the map, which
start landmarks (or are dropped when the map is full).  Each figure is the
median of ``reps`` calls after one warm-up, each from the freshly placed state;
min and max follow in brackets."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-robot_simu_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

CAP, K_HELD, K_FAR = 10000, 18, 2


def world():
    import ekf_oracle as eo
    rs = np.random.RandomState(5)
    g = np.arange(100) * 4.0 - 198.0
    xy = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2) + rs.uniform(-1, 1, (CAP, 2))
    lm = np.column_stack([xy, rs.uniform(-np.pi, np.pi, CAP)])
    pose = np.array([1.0, 0.5, 0.7])
    lm = lm[np.argsort(np.hypot(lm[:, 0] - pose[0], lm[:, 1] - pose[1]), kind="stable")]
    prior = lm + rs.normal(0, 0.05, lm.shape)
    obs = np.array([eo.scan_predict(pose, lm[j]) for j in range(K_HELD)])
    obs[:, 0] *= 1 + 0.01 * rs.standard_normal(K_HELD)
    obs = np.vstack([obs, [[900.0, 0.3, 0.1], [950.0, -2.0, 1.0]]])
    return pose, prior, obs


def fmt(v):
    v = np.asarray(v) * 1e3
    return f"{np.median(v):9.1f} [{v.min():.1f} .. {v.max():.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ekfslam_assoc_ab.txt"))
    args = ap.parse_args()
    from slamhip.ekf import DeviceEKFSLAM
    pose, prior, obs = world()
    n = 3 + 3 * CAP
    lines = [f"slam_ekfslam_observe, capacity {CAP} (n = {n}), k = {K_HELD + K_FAR} "
             f"({K_HELD} of held landmarks, {K_FAR} beyond the map); device time in us, "
             f"median of {args.reps} [min .. max]", ""]
    known = DeviceEKFSLAM(CAP)
    assoc = DeviceEKFSLAM(CAP, association="ml", p_new=1e-4)
    try:
        for count in (100, 1000, 10000):
            na = 3 + 3 * count
            mu, diag = np.zeros(n), np.zeros(n)
            mu[:3], diag[:3] = pose, (1e-4, 1e-4, 1e-5)
            mu[3:na], diag[3:na] = prior[:count].ravel(), 0.01
            rows = {q: [] for q in ("scan_ms", "assign_ms", "update_ms", "init_ms")}
            for rep in range(args.reps + 1):
                assoc.init_diag(mu, diag)
                assoc.set_count(count)
                a = assoc.observe(obs)
                if rep:
                    for q, v in assoc.assoc_timing().items():
                        rows[q].append(v)
            info = assoc.assoc_info()
            m = np.flatnonzero(a >= 0)
            mu_k, diag_k = mu.copy(), diag.copy()
            mu_k[3:], diag_k[3:] = prior.ravel(), 0.01
            upd = []
            for rep in range(args.reps + 1):
                known.init_diag(mu_k, diag_k)
                known.update(a[m], obs[m])
                if rep:
                    t = known.timing()
                    upd.append(t["gather_ms"] + t["inverse_ms"] + t["gain_ms"] + t["rank_update_ms"])
            lines += [f"count = {count}: matched {info['matched']}, new {info['new']}, dropped "
                      f"{info['dropped']}; update tiles {info['tiles']} of {known.info()['n_tiles']}",
                      f"  scan        {fmt(rows['scan_ms'])}",
                      f"  assign      {fmt(rows['assign_ms'])}",
                      f"  update      {fmt(rows['update_ms'])}",
                      f"  initialise  {fmt(rows['init_ms'])}",
                      f"  known-id update, same matches, all {n} rows  {fmt(upd)}", ""]
    finally:
        assoc.close()
        known.close()
    text = "\n".join(lines)
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
