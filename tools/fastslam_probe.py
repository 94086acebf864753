"""FastSLAM's phases on the device, and its map gather against a plain copy.

Workload: NL = 100 landmarks, every one seen after the first step, k = 10
observations per step after that, linear motion, device RNG, ESS_TH = NP so
that every step resamples (the gather moves 100 landmarks' rows: 2 x 40 B x 100
x NP of traffic).  For NP in {2^12, 2^16, 2^20}, after WARM untimed steps, the
median over REPS steps of

  * slam_fs_timing's four phases (HIP events): map gather, predict, map update
    + weights, step end; and the wall-clock of the whole step call;
  * the map gather's bytes per second against a device-to-device copy of the
    same byte count (torch, timed with events in this probe) and against 8 TB/s;
  * a DeviceParticleFilter step at the same NP with NL = k = 10 known landmarks
    (the localisation-only cost of the same observations), wall-clock.

Writes profiles/fastslam_ab.txt.  Usage: python tools/fastslam_probe.py [REPS [OUT]]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-robot_simu_amd"))
import torch  # noqa: E402
from slamhip.fastslam import DeviceFastSLAM  # noqa: E402
from slamhip.pf import DeviceParticleFilter  # noqa: E402

NL, K, WARM = 100, 10, 3
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
OUT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "fastslam_ab.txt")
NOISE = (0.1, np.deg2rad(3.0), np.deg2rad(3.0))
CTL = (10.0 * np.deg2rad(10.0), np.deg2rad(10.0))


def observations(rs, lm, pose, ids):
    psi = np.pi / 2 - pose[2]
    c, s = np.cos(psi), np.sin(psi)
    dx, dy = lm[ids, 0] - pose[0], lm[ids, 1] - pose[1]
    rx, ry = c * dx - s * dy, s * dx + c * dy
    g = rs.standard_normal((len(ids), 3))
    return np.column_stack([np.hypot(rx, ry) * (1 + NOISE[0] * g[:, 0]),
                            np.arctan2(ry, rx) + NOISE[1] * g[:, 1], psi + NOISE[2] * g[:, 2]])


def advance(pose, dt=0.1):
    """The reference's linear model (particle_filter.py:121-142), noise free."""
    return np.array([pose[0] + CTL[0] * dt * np.cos(pose[2]), pose[1] + CTL[0] * dt * np.sin(pose[2]),
                     pose[2] + CTL[1] * dt])


def copy_ms(nbytes):
    """Device-to-device copy of nbytes (read nbytes, write nbytes)."""
    a = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    a.fill_(1.0)
    ts = []
    for _ in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts[WARM:]))


def main():
    rs = np.random.RandomState(1)
    lm = rs.uniform(-12, 12, (NL, 2))
    lines = [f"FastSLAM probe: NL = {NL}, k = {K}, every step resamples, median of {REPS} steps",
             "ms: gather / predict / map update + weights / step end (HIP events); step, pf: wall-clock"]
    for lg in (12, 16, 20):
        n = 1 << lg
        pose = advance(np.array([10.0, 0.0, np.pi / 2]))
        with DeviceFastSLAM(n, NL, noise=NOISE, ess_threshold=float(n), seed=1) as fs:
            fs.step(CTL, np.arange(NL), observations(rs, lm, pose, np.arange(NL)))
            rows, walls = [], []
            for r in range(WARM + REPS):
                pose = advance(pose)
                ids = (np.arange(K) * 7 + 3 * r) % NL
                obs = observations(rs, lm, pose, ids)
                t0 = time.perf_counter()
                out = fs.step(CTL, ids, obs)
                walls.append((time.perf_counter() - t0) * 1e3)
                assert out["resampled"] and fs.info()["n_seen"] == NL
                rows.append(list(fs.timing().values()))
            ph = np.median(np.array(rows[WARM:]), axis=0)
            wall = float(np.median(walls[WARM:]))
        gbytes = 2 * 40 * NL * n
        cms = copy_ms(gbytes // 2)
        with DeviceParticleFilter(n, lm[:K], ess_threshold=float(n), seed=1) as pf:
            z = rs.uniform(-5, 5, (K, 2))
            t = []
            for _ in range(WARM + REPS):
                t0 = time.perf_counter()
                pf.step(CTL, z)
                t.append((time.perf_counter() - t0) * 1e3)
            pf_ms = float(np.median(t[WARM:]))
        gbs = gbytes / (ph[0] * 1e-3) / 1e12
        cbs = gbytes / (cms * 1e-3) / 1e12
        lines.append(f"NP=2^{lg}: gather {ph[0]:.4f}  predict {ph[1]:.4f}  update {ph[2]:.4f}  "
                     f"end {ph[3]:.4f}  step {wall:.4f}  pf(NL={K}) {pf_ms:.4f}  "
                     f"step/pf {wall / pf_ms:.2f}")
        lines.append(f"         gather {gbytes / 1e6:.1f} MB: {gbs:.3f} TB/s; copy of the same bytes "
                     f"{cms:.4f} ms = {cbs:.3f} TB/s; gather/copy {gbs / cbs:.2f}; "
                     f"of 8 TB/s {gbs / 8:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
