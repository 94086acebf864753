"""FastSLAM 2.0 without ids: the associating proposal launch beside its two
parents, and against a plain copy of the bytes its scan reads.

Workload (tools/fastslam_assoc_probe.py's grid): a world of NL landmarks (25 and
100), capacity NL + 8, a first step that observes every landmark (every particle
starts NL landmarks), then k = 10 observations per step of true landmarks,
linear motion, device RNG, ESS_TH = NP so that every step resamples.  Three
handles step the same observations in turn in the same process: the new one
(association="ml_marginal", proposal="measurement"), an "ml" 1.0 handle and a
known-id 2.0 handle.  For NP in {2^12, 2^16, 2^20}, after WARM untimed steps,
the median over REPS steps of

  * HIP-event ms of fs_assoc_proposal_kernel (slam_fs_timing's "predict" on the
    new handle), of the 1.0 handle's association update + weights ("update") and
    of the known-id 2.0 handle's fs_proposal_kernel ("predict"); the wall-clock
    of the whole step call of all three;
  * the bytes the scan reads, 44 B x cnt x k x NP (five map components and the
    stamp per candidate), against a device-to-device copy moving the same byte
    count (torch, timed with events here) and against 8 TB/s;
  * candidate evaluations per second.

Writes profiles/fastslam2_assoc_ab.txt.
Usage: python tools/fastslam2_assoc_probe.py [REPS [OUT [LOG2NP ...]]]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-robot_simu_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402,F401
from fastslam_assoc_probe import copy_ms  # noqa: E402
from fastslam_probe import CTL, NOISE, advance, observations  # noqa: E402
from slamhip.fastslam import DeviceFastSLAM  # noqa: E402

K, WARM, SPARE = 10, 3, 8
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
OUT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else \
    os.path.join(ROOT, "profiles", "fastslam2_assoc_ab.txt")
LOGS = [int(v) for v in sys.argv[3:]] or [12, 16, 20]


def main():
    lines = [f"FastSLAM 2.0 association probe: k = {K}, every step resamples, median of {REPS} steps",
             "ms (HIP events): 2.0-ml = fs_assoc_proposal_kernel, 1.0-ml = association update + "
             "weights, 2.0-known = fs_proposal_kernel; step: wall-clock of the whole call"]
    for nl in (25, 100):
        lm = np.random.RandomState(1).uniform(-12, 12, (nl, 2))
        for lg in LOGS:
            n = 1 << lg
            rs = np.random.RandomState(2)
            kw = dict(noise=NOISE, ess_threshold=float(n), seed=1)
            with DeviceFastSLAM(n, nl + SPARE, association="ml_marginal", proposal="measurement",
                                **kw) as new, \
                    DeviceFastSLAM(n, nl + SPARE, association="ml", **kw) as ml1, \
                    DeviceFastSLAM(n, nl, proposal="measurement", **kw) as kn2:
                hs = (("new", new, False, 1), ("ml1", ml1, False, 2), ("kn2", kn2, True, 1))
                pose = advance(np.array([10.0, 0.0, np.pi / 2]))
                every = np.arange(nl)
                first = observations(rs, lm, pose, every)
                for _, fs, known, _ in hs:
                    fs.step(CTL, every if known else None, first)
                ev = {t: [] for t, *_ in hs}
                walls = {t: [] for t, *_ in hs}
                for r in range(WARM + REPS):
                    pose = advance(pose)
                    ids = (np.arange(K) * 7 + 3 * r) % nl
                    obs = observations(rs, lm, pose, ids)
                    for tag, fs, known, phase in hs:
                        t0 = time.perf_counter()
                        out = fs.step(CTL, ids if known else None, obs)
                        walls[tag].append((time.perf_counter() - t0) * 1e3)
                        # (a 2.0 handle's first step leaves equal weights, ESS = NP exactly:
                        # its resampling starts one step later, inside the warm-up)
                        assert out["resampled"] or r < WARM
                        ev[tag].append(list(fs.timing().values())[phase])
                cnt = new.get_counts()
                cnt1 = ml1.get_counts()
            ms = {t: float(np.median(v[WARM:])) for t, v in ev.items()}
            wall = {t: float(np.median(v[WARM:])) for t, v in walls.items()}
            mean_cnt = float(cnt.mean())
            cand = mean_cnt * K * n
            sbytes = 44.0 * cand
            cms = copy_ms(int(44 * mean_cnt * n) // 2, K)
            sbs = sbytes / (ms["new"] * 1e-3) / 1e12
            lines.append(f"NL={nl} NP=2^{lg}: counts {cnt.min()}..{cnt.max()} (mean {mean_cnt:.2f}; "
                         f"1.0-ml {cnt1.min()}..{cnt1.max()})")
            lines.append(f"   launch ms: 2.0-ml {ms['new']:.4f}  1.0-ml {ms['ml1']:.4f}  2.0-known "
                         f"{ms['kn2']:.4f}   2.0-ml/1.0-ml {ms['new'] / ms['ml1']:.2f}  "
                         f"2.0-ml/2.0-known {ms['new'] / ms['kn2']:.1f}")
            lines.append(f"   step ms:   2.0-ml {wall['new']:.4f}  1.0-ml {wall['ml1']:.4f}  2.0-known "
                         f"{wall['kn2']:.4f}")
            lines.append(f"   scan reads {sbytes / 1e6:.1f} MB: {sbs:.3f} TB/s; copy of the same bytes "
                         f"{cms:.4f} ms; scan/copy time {ms['new'] / cms:.2f}; of 8 TB/s {sbs / 8:.3f}; "
                         f"{cand / (ms['new'] * 1e-3) / 1e9:.2f} G candidates/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
