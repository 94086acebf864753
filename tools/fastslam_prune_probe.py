"""The evidence pass (fs_prune_kernel) on the device: what it costs beside the
update it follows, and what the smaller maps give back.

On tools/fastslam_assoc_probe.py's grid -- NL in {25, 100} x NP in {2^12, 2^16,
2^20}, k = 10, every particle holding NL landmarks, median of REPS -- for an
"ml" handle of capacity NL + 8:

  * the pass with nothing removed and with every second slot removed: HIP-event
    ms of slam_fs_timing's phase 2 on a k = 0 step (no update is launched: the
    4 B x NP copy of the counts, the pass and its fold), beside a
    device-to-device copy of the bytes the case moves -- 24 B read and 4 B
    written per live slot, 24 B more read and 40 B more written per moved slot,
    36 B read and 16 B written per particle (pose, counts, removed, the copy);
  * the update launch on the same handle and state: phase 2 of a k = 10 step
    with pruning off, and with pruning on (update + pass);
  * the steady state: tools/fastslam_pnew_sweep.py's world at p_new = 0.1, 100
    steps at NP = 2^16 with pruning on and off -- phase 2 and the mean count at
    the last step.

Every case runs in a child process under its own time limit; the first failure
stops the probe.  Writes profiles/fastslam_prune_ab.txt.
Usage: python tools/fastslam_prune_probe.py [REPS [OUT [LOG2NP ...]]]
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-robot_simu_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

K, WARM, SPARE = 10, 3, 8
CASE_LIMIT_S = 240


def _median_phase2(fs, reps, prepare, step):
    ts = []
    for _ in range(WARM + reps):
        prepare()
        step()
        ts.append(fs.timing()["map_update"])
    return float(np.median(ts[WARM:]))


def copy_ms(nbytes, reps):
    """A device-to-device copy that reads nbytes / 2 and writes nbytes / 2."""
    import torch
    a = torch.empty(max(1, nbytes // 16), dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    a.fill_(1.0)
    ts = []
    for _ in range(WARM + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts[WARM:]))


def case(nl, lg, reps):
    """One grid point, in this process."""
    from fastslam_probe import CTL, NOISE, advance, observations
    from slamhip.fastslam import DeviceFastSLAM
    n, cap = 1 << lg, nl + SPARE
    lm = np.random.RandomState(1).uniform(-12, 12, (nl, 2))
    rs = np.random.RandomState(2)
    pose = advance(np.array([10.0, 0.0, np.pi / 2]))
    every = np.arange(nl)
    cnt = np.full(n, nl, dtype=np.int32)
    keep = np.full((n, cap), 5, dtype=np.int32)
    half = keep.copy()
    half[:, 1::2] = -5
    prune = dict(view_range=1e-3, init=1, hit=0, miss=1, remove_below=0)     # nothing is in view
    with DeviceFastSLAM(n, cap, association="ml", noise=NOISE, ess_threshold=0.0, seed=1,
                        prune=prune) as fs:
        fs.step(CTL, None, observations(rs, lm, pose, every))
        assert (fs.get_counts() == nl).all()
        empty = np.zeros((0, 3))
        obs = observations(rs, lm, advance(pose), (np.arange(K) * 7) % nl)

        def load(ev):
            def f():
                fs.set_counts(cnt)
                fs.set_evidence(ev)
            return f
        t_none = _median_phase2(fs, reps, load(keep), lambda: fs.step(CTL, None, empty))
        assert not fs.last_removed().any()
        t_half = _median_phase2(fs, reps, load(half), lambda: fs.step(CTL, None, empty))
        removed = int(fs.last_removed()[0])
        assert removed == nl // 2 and (fs.get_counts() == nl - removed).all()
        # the same preparation on both sides (set_counts alone: on the pruning handle it also
        # puts the evidence at init, and with nothing in view nothing is removed)
        t_both = _median_phase2(fs, reps, lambda: fs.set_counts(cnt), lambda: fs.step(CTL, None, obs))
        assert not fs.last_removed().any()
        fs.set_pruning(None)
        t_upd = _median_phase2(fs, reps, lambda: fs.set_counts(cnt), lambda: fs.step(CTL, None, obs))
    kept = nl - removed
    per_particle = 36 + 16
    b_none = n * (28 * nl + per_particle)
    b_half = n * (24 * nl + 4 * kept + 64 * (kept - 1) + per_particle)
    return dict(nl=nl, lg=lg, t_none=t_none, t_half=t_half, t_both=t_both, t_upd=t_upd,
                b_none=b_none, b_half=b_half, c_none=copy_ms(b_none, reps),
                c_half=copy_ms(b_half, reps), removed=removed)


def steady(lg):
    """The sweep world, pruning on and off: phase 2 and the counts at step 100."""
    from fastslam_pnew_sweep import NOISE, world
    from slamhip.fastslam import DeviceFastSLAM
    n = 1 << lg
    ctl, scans, n_obs, _ = world(0)
    out = dict(lg=lg, observed=n_obs)
    for tag, prune in (("off", None), ("on", dict(view_range=7.2))):
        with DeviceFastSLAM(n, 32, association="ml", p_new=0.1, noise=NOISE,
                            q=np.diag([0.03, 0.03, np.deg2rad(2.0)]) ** 2, ess_threshold=n / 2.0,
                            seed=1, prune=prune) as fs:
            ts = []
            for obs in scans:
                r = fs.step(ctl, None, obs)
                ts.append(fs.timing()["map_update"])
            cnt = fs.get_counts()
            out[tag] = dict(last=float(np.median(ts[-10:])), mean_cnt=float(cnt.mean()),
                            max_cnt=int(cnt.max()), best_cnt=int(cnt[r["max_idx"]]))
    return out


def child(args):
    """Run one case in a fresh process under its own time limit."""
    p = subprocess.run(["timeout", "-k", "10", str(CASE_LIMIT_S), sys.executable,
                        os.path.abspath(__file__), "9", "-", "--case"] + [str(a) for a in args],
                       capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"case {args} failed with status {p.returncode}: the probe stops here")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 3 and sys.argv[3] == "--case":      # a child: REPS OUT --case ...
        a = sys.argv[4:]
        res = steady(int(a[1])) if a[0] == "steady" else case(int(a[0]), int(a[1]), int(a[2]))
        print(json.dumps(res))
        return
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    out = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else \
        os.path.join(ROOT, "profiles", "fastslam_prune_ab.txt")
    logs = [int(v) for v in sys.argv[3:]] or [12, 16, 20]
    lines = [f"FastSLAM evidence pass probe: k = {K}, median of {reps}; HIP-event ms of phase 2",
             "pass: k = 0 step (counts copy + fs_prune_kernel + fold); copy: device-to-device copy "
             "of the bytes the case moves"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    for nl in (25, 100):
        for lg in logs:
            r = child([nl, lg, reps])
            emit(f"NL={nl} NP=2^{lg}: pass, none removed {r['t_none']:.4f} ms "
                 f"({r['b_none'] / 1e6:.1f} MB, copy {r['c_none']:.4f} ms, pass/copy "
                 f"{r['t_none'] / r['c_none']:.2f}); every second slot removed ({r['removed']}) "
                 f"{r['t_half']:.4f} ms ({r['b_half'] / 1e6:.1f} MB, copy {r['c_half']:.4f} ms, "
                 f"pass/copy {r['t_half'] / r['c_half']:.2f})")
            emit(f"   update launch, pruning off {r['t_upd']:.4f} ms; update + pass {r['t_both']:.4f} ms; "
                 f"pass / update {r['t_none'] / r['t_upd']:.3f}")
    s = child(["steady", 16, 0])
    emit(f"steady state, sweep world seed 0, p_new 0.1, NP=2^{s['lg']}, {s['observed']} landmarks observed, "
         "phase 2 over the last 10 of 100 steps:")
    for tag in ("off", "on"):
        v = s[tag]
        emit(f"   pruning {tag}: {v['last']:.4f} ms, mean count {v['mean_cnt']:.2f}, largest "
             f"{v['max_cnt']}, best particle's {v['best_cnt']}")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
