"""Everything the particle filter's step end produces, for a bitwise A/B of two
builds of the library (development tool).

    SLAM_HIP_LIB=.../libslam_A.so python tools/step_end_dump.py a.npz
    SLAM_HIP_LIB=.../libslam_B.so python tools/step_end_dump.py b.npz
    python tools/step_end_dump.py --compare a.npz b.npz

One process per library.  Dumped, per run: every field of every record,
get_weights_raw, get_state, and the indices slam_pf_resample_indices draws
from the final weights.  Runs: 512, 1,000, 12,345, 524,800 and 2^20 particles,
each stepwise (full step ends) and as batches of 5 + 8 steps (split step
ends), with the world and the ESS threshold of tests/test_gpu_finalize_split.py
(every other step resamples, so the block prefix the step end leaves for the
exact cumsum shows in the state); the same with step 7 degenerate at 12,345;
2^21 + 12,345 (the fast kernel behind the slice pre-pass) and 2^24 + 12,345
(the general kernel) as batches; one DistFilter(world=1) run.  The comparison
is by bytes, so NaNs compare by bit pattern.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-robot_simu_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), "different sets of arrays"
    bad, values = [], 0
    for k in a.files:
        x, y = a[k], b[k]
        values += x.size
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(k)
    print(f"{len(a.files)} arrays, {values} values compared; differing arrays: {len(bad)}")
    for k in bad:
        print("  DIFFERS", k)
    return 1 if bad else 0


def dump(path):
    import test_gpu_finalize_split as fsplit
    from slamhip.dist import DistFilter
    out = {}

    def put(tag, recs, pf, raw=True):
        for name in recs.dtype.names:
            out[f"{tag}/rec/{name}"] = np.ascontiguousarray(recs[name])
        if raw:
            w_un, s = pf.get_weights_raw()
            out[f"{tag}/w_un"], out[f"{tag}/s"] = w_un, np.array([s])
        for nm, v in zip("xytw", pf.get_state()):
            out[f"{tag}/state/{nm}"] = v
        if raw:
            idx, ns = pf.resample_indices(0.37)
            out[f"{tag}/resample_idx"], out[f"{tag}/n_special"] = idx, np.array([ns])
        print(tag, "resampled", recs["resampled"].tolist(), flush=True)

    steps, split_at = fsplit.STEPS, fsplit.SPLIT_AT
    ctl = np.tile([fsplit.VEL, fsplit.OMEGA], (steps, 1))

    def both(n, tag, edit=None, stepwise=True):
        lm, zs = fsplit._world()
        if edit is not None:
            edit(zs)
        pf = fsplit._filter(n, lm, zs)
        recs = np.concatenate([pf.run(0, ctl[:split_at]).records.copy(),
                               pf.run(split_at, ctl[split_at:]).records.copy()])
        put(f"{tag}/batch", recs, pf)
        pf.close()
        if stepwise:
            pf = fsplit._filter(n, lm, zs)
            recs = np.concatenate([pf.run(k, ctl[k:k + 1]).records.copy() for k in range(steps)])
            put(f"{tag}/stepwise", recs, pf)
            pf.close()

    for n in (512, 1000, 12345, 524800, 1 << 20):
        both(n, f"n{n}")

    def degenerate(zs):
        zs[7] = 1e3
    both(12345, "n12345_degenerate", degenerate)
    both((1 << 21) + 12345, "n2p21")
    both((1 << 24) + 12345, "n2p24", stepwise=False)

    lm, zs = fsplit._world()
    d = DistFilter(1 << 20, lm, world=1, dt=fsplit.DT, motion="velocity", likelihood="logsum",
                   seed=4321, ess_threshold=fsplit.ESS_FRAC * (1 << 20))
    d.load_observations(zs)
    recs = np.concatenate([d.run(0, ctl[:split_at]).records.copy(),
                           d.run(split_at, ctl[split_at:]).records.copy()])
    put("dist_world1", recs, d, raw=False)
    d.close()
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    dump(sys.argv[1])
