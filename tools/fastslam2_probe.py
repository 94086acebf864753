"""FastSLAM 2.0's proposal launch beside the FastSLAM 1.0 step, and against a
plain copy of the bytes it moves.

Workload (tools/fastslam_probe.py's): NL = 100 landmarks, every one seen after
the first step, k = 10 observations per step after that, linear motion, device
RNG, ESS_TH = NP so that every step resamples.  A 1.0 handle and a 2.0 handle
step in turn in the same process.  For NP in {2^12, 2^16, 2^20}, after WARM
untimed steps, the median over REPS steps of

  * slam_fs_timing's four phases (HIP events) of both handles.  On the 2.0
    handle "predict" is fs_proposal_kernel (motion + proposal + sampling + map
    update in one launch) and "update" the weights alone;
  * the wall-clock of the whole step call of both;
  * the bytes fs_proposal_kernel moves, from its layout: per particle 24 B of
    pose and 8 B of weight read, 24 + 8 + 8 B of pose, weight and L written,
    and per seen observation 40 B of map row read by the proposal pass, 40 B
    read again and 40 B written by the map pass (a first sighting: 40 B
    written) --
        bytes = NP (72 + 120 k_seen + 40 k_unseen);
    a recording handle adds 72 NP, host noise 24 NP;
  * a device-to-device copy of that byte count (torch, timed with events in
    this probe), and the ratios proposal / copy and proposal / (1.0 predict +
    1.0 update).

Writes profiles/fastslam2_ab.txt.  Usage: python tools/fastslam2_probe.py [REPS [OUT]]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-robot_simu_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402,F401
from fastslam_probe import CTL, NOISE, advance, observations  # noqa: E402
from slamhip.fastslam import DeviceFastSLAM  # noqa: E402

NL, K, WARM = 100, 10, 3
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
OUT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else \
    os.path.join(ROOT, "profiles", "fastslam2_ab.txt")


def proposal_bytes(n, k_seen, k_unseen=0):
    return n * (72 + 120 * k_seen + 40 * k_unseen)


def copy_ms(nbytes):
    """Device-to-device copy moving nbytes in all (reads half, writes half)."""
    a = torch.empty(nbytes // 16, dtype=torch.float64, device="cuda")
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
    lines = [f"FastSLAM 2.0 probe: NL = {NL}, k = {K}, every step resamples, median of {REPS} steps",
             "ms: gather / predict / update / step end (HIP events); step: wall-clock.  2.0: predict = "
             "fs_proposal_kernel, update = weights alone"]
    for lg in (12, 16, 20):
        n = 1 << lg
        pose = advance(np.array([10.0, 0.0, np.pi / 2]))
        kw = dict(noise=NOISE, ess_threshold=float(n), seed=1)
        with DeviceFastSLAM(n, NL, **kw) as one, \
                DeviceFastSLAM(n, NL, proposal="measurement", **kw) as two:
            first = observations(rs, lm, pose, np.arange(NL))
            rows, walls = {1: [], 2: []}, {1: [], 2: []}
            for fs in (one, two):
                fs.step(CTL, np.arange(NL), first)
            for r in range(WARM + REPS):
                pose = advance(pose)
                ids = (np.arange(K) * 7 + 3 * r) % NL
                obs = observations(rs, lm, pose, ids)
                for tag, fs in ((1, one), (2, two)):
                    t0 = time.perf_counter()
                    out = fs.step(CTL, ids, obs)
                    walls[tag].append((time.perf_counter() - t0) * 1e3)
                    # (the 2.0 handle's first step leaves equal weights, ESS = NP exactly:
                    # its resampling starts one step later, inside the warm-up)
                    assert (out["resampled"] or r < WARM) and fs.info()["n_seen"] == NL
                    rows[tag].append(list(fs.timing().values()))
            ph = {t: np.median(np.array(rows[t][WARM:]), axis=0) for t in (1, 2)}
            wall = {t: float(np.median(walls[t][WARM:])) for t in (1, 2)}
        nbytes = proposal_bytes(n, K)
        cms = copy_ms(nbytes)
        for t, name in ((1, "1.0"), (2, "2.0")):
            lines.append(f"NP=2^{lg} {name}: gather {ph[t][0]:.4f}  predict {ph[t][1]:.4f}  "
                         f"update {ph[t][2]:.4f}  end {ph[t][3]:.4f}  step {wall[t]:.4f}")
        lines.append(f"         proposal launch {nbytes / 1e6:.2f} MB = NP (72 + 120 k): "
                     f"{nbytes / (ph[2][1] * 1e-3) / 1e12:.3f} TB/s; copy of the same bytes {cms:.4f} ms; "
                     f"proposal/copy {ph[2][1] / cms:.2f}; proposal/(1.0 predict + update) "
                     f"{ph[2][1] / (ph[1][1] + ph[1][2]):.2f}; step 2.0/1.0 {wall[2] / wall[1]:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
