"""Phase timeline of the 2^20 finalize (development tool, round 6): runs the C2
workload through a probe build (tools/build_variant.sh finprobe -DSLAM_FIN_PROBE)
two steps per batch and prints the finalize's wall-clock stamps (thread 0)
for the split step end (the first step) and the full one (the batch's last):
loads + np.sum rounds, the last buffer chain + rescale + candidates, the
sums + argmax + record, the record / counters, the next step's block prefix;
and when each moment workgroup of the split step end finished."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "slam-robot_simu_amd"))
os.environ.setdefault("SLAM_HIP_LIB", os.path.join(ROOT, "slam-robot_simu_amd/slamhip/libslam_finprobe.so"))
import bench  # noqa: E402
from slamhip.pf import DeviceParticleFilter  # noqa: E402

lib = C.CDLL(os.environ["SLAM_HIP_LIB"])
buf = (C.c_longlong * 32)()
n = int(os.environ.get("FP_N", str(1 << 20)))
lm, zs, (vel, omega, dt) = bench.simulate_world(700)
ctl = np.tile([vel, omega], (700, 1))
pf = DeviceParticleFilter(n, lm, dt=dt, motion="velocity", likelihood="logsum", seed=1234)
pf.load_observations(zs)
bench.settle(pf.run, ctl, 310)
names = ["loads+rounds", "chain+cand", "sums+argmax", "record", "prefix"]
# two steps per batch: the first takes the split step end (workgroup 0's
# stamps at [16..21], moment workgroup g's end at [24 + g]), the second, the
# batch's last, the full one (stamps at [0..5]); a library without the split
# stamps only [0..5], for the batch's last step
rows = {"full": [], "split": []}
mom_end = []
for k in range(310, 430, 2):
    out = pf.run(k, ctl[k:k + 2])
    assert lib.slam_fin_probe_read(buf) == 0
    t = np.array(buf[:32], dtype=np.float64) * 0.01             # us (100 MHz)
    rows["full"].append((np.diff(t[0:6]), out[1]["resample_next"]))
    if buf[16]:
        rows["split"].append((np.diff(t[16:22]), out[0]["resample_next"]))
        mom_end.append((t[24:32][np.array(buf[24:32]) != 0] - t[16], t[21] - t[16], out[0]["resample_next"]))
for path in ("full", "split"):
    for flag in (False, True):
        sel = [r for r, f in rows[path] if f == flag]
        if sel:
            med = np.median(np.array(sel), axis=0)
            print(f"{path} resample_next={flag} ({len(sel)} steps): "
                  + "  ".join(f"{a} {b:5.2f}" for a, b in zip(names, med)) + f"  | total {med.sum():5.2f} us")
for flag in (False, True):
    sel = [(m, e) for m, e, f in mom_end if f == flag]
    if sel:
        m = np.array([x for x, _ in sel])
        e = np.array([x for _, x in sel])
        late = int(np.sum(m.max(axis=1) > e))
        print(f"split resample_next={flag}: moment workgroups end (us after workgroup 0's start) median "
              + " ".join(f"{v:5.2f}" for v in np.median(m, axis=0)) + f"  max {m.max():5.2f}"
              + f"  | workgroup 0 ends {np.median(e):5.2f} (min {e.min():5.2f}); "
              f"steps with a moment workgroup ending later: {late} of {len(sel)}")
