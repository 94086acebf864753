"""The association update on the device against three references.

Workload: a world of NL landmarks (25 and 100), an associating handle of
capacity NL + 8 whose first step observes every landmark (every particle starts
NL landmarks), then k = 10 observations per step of true landmarks, linear
motion, device RNG, ESS_TH = NP so that every step resamples.  For NP in
{2^12, 2^16, 2^20}, after WARM untimed steps, the median over REPS steps of

  * slam_fs_timing's four phases (HIP events) and the wall-clock of the step;
  * the same on a known-association handle stepping the same observations with
    their true ids (what the association costs over being told);
  * the bytes the scan reads, 44 B x cnt x k x NP (five map components and the
    stamp per candidate), per second, against a device-to-device copy moving
    the same byte count (torch, timed with events here) and against 8 TB/s;
  * candidate evaluations per second.

Writes profiles/fastslam_assoc_ab.txt.
Usage: python tools/fastslam_assoc_probe.py [REPS [OUT [LOG2NP ...]]]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-robot_simu_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from fastslam_probe import CTL, NOISE, advance, observations  # noqa: E402
from slamhip.fastslam import DeviceFastSLAM  # noqa: E402

K, WARM, SPARE = 10, 3, 8
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
OUT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else \
    os.path.join(ROOT, "profiles", "fastslam_assoc_ab.txt")
LOGS = [int(v) for v in sys.argv[3:]] or [12, 16, 20]


def copy_ms(nbytes, times):
    """`times` device-to-device copies of nbytes (each reads nbytes, writes nbytes)."""
    a = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    a.fill_(1.0)
    ts = []
    for _ in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(times):
            b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts[WARM:]))


def run(fs, rs, lm, known):
    nl = len(lm)
    pose = advance(np.array([10.0, 0.0, np.pi / 2]))
    every = np.arange(nl)
    fs.step(CTL, every if known else None, observations(rs, lm, pose, every))
    rows, walls = [], []
    for r in range(WARM + REPS):
        pose = advance(pose)
        ids = (np.arange(K) * 7 + 3 * r) % nl
        obs = observations(rs, lm, pose, ids)
        t0 = time.perf_counter()
        out = fs.step(CTL, ids if known else None, obs)
        walls.append((time.perf_counter() - t0) * 1e3)
        assert out["resampled"]
        rows.append(list(fs.timing().values()))
    return np.median(np.array(rows[WARM:]), axis=0), float(np.median(walls[WARM:]))


def main():
    lines = [f"FastSLAM association probe: k = {K}, every step resamples, median of {REPS} steps",
             "ms: gather / predict / map update + weights / step end (HIP events); step: wall-clock"]
    for nl in (25, 100):
        lm = np.random.RandomState(1).uniform(-12, 12, (nl, 2))
        for lg in LOGS:
            n = 1 << lg
            kw = dict(noise=NOISE, ess_threshold=float(n), seed=1)
            with DeviceFastSLAM(n, nl + SPARE, association="ml", **kw) as fs:
                ph, wall = run(fs, np.random.RandomState(2), lm, False)
                cnt = fs.get_counts()
            with DeviceFastSLAM(n, nl, **kw) as fk:
                pk, wallk = run(fk, np.random.RandomState(2), lm, True)
            mean_cnt = float(cnt.mean())
            cand = mean_cnt * K * n
            sbytes = 44.0 * cand
            cms = copy_ms(int(44 * mean_cnt * n) // 2, K)
            sbs = sbytes / (ph[2] * 1e-3) / 1e12
            cbs = sbytes / (cms * 1e-3) / 1e12
            lines.append(f"NL={nl} NP=2^{lg}: counts {cnt.min()}..{cnt.max()} (mean {mean_cnt:.2f})")
            lines.append(f"   ml:    gather {ph[0]:.4f}  predict {ph[1]:.4f}  update {ph[2]:.4f}  "
                         f"end {ph[3]:.4f}  step {wall:.4f}")
            lines.append(f"   known: gather {pk[0]:.4f}  predict {pk[1]:.4f}  update {pk[2]:.4f}  "
                         f"end {pk[3]:.4f}  step {wallk:.4f}   update ml/known {ph[2] / pk[2]:.1f}  "
                         f"step ml/known {wall / wallk:.2f}")
            lines.append(f"   scan reads {sbytes / 1e6:.1f} MB: {sbs:.3f} TB/s; copy of the same bytes "
                         f"{cms:.4f} ms = {cbs:.3f} TB/s; scan/copy time {ph[2] / cms:.2f}; "
                         f"of 8 TB/s {sbs / 8:.3f}; {cand / (ph[2] * 1e-3) / 1e9:.2f} G candidates/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
