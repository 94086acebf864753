"""Many reference-size particle filters at once: the ensemble (one launch per
run, one workgroup per filter) against what the library offered before.

Workload: NP = 1000 particles, NL = 20 landmarks, velocity motion model, device
RNG, product likelihood, 64 steps per `run` call; every row is timed after one
untimed run of the same call (graphs captured, buffers allocated), REPS times,
median wall-clock of the whole call (host copies and the wait included) and,
for the ensemble, the HIP-event time of its launch.

  (a) BatchParticleFilter, B in {64, 1024, 4096}
  (b) the same 64 filters as 64 DeviceParticleFilter handles, each `run` for 64
      steps, one after another
  (c) one DeviceParticleFilter of 64 000 and of 1 024 000 particles (the same
      particle count without the independence)

Writes profiles/ensemble_ab.txt.  Usage: python tools/ensemble_probe.py [REPS [OUT]]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "slam-robot_simu_amd"))
import pf_oracle as po  # noqa: E402
from slamhip.pf import DeviceParticleFilter  # noqa: E402
from slamhip.pf_batch import BatchParticleFilter  # noqa: E402

NP, NL, STEPS = 1000, 20, 64
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ensemble_ab.txt")


def world():
    rs = np.random.RandomState(1)
    lm = rs.uniform(-10, 10, (NL, 2))
    p = po.PFParams(n_particles=NP, landmarks=lm, motion="velocity")
    w = po.PFWorld(p)
    zs = []
    for _ in range(STEPS):
        xt = w.advance()
        zs.append(po.to_robot_frame(xt, lm) + rs.multivariate_normal([0.0, 0.0], p.r, NL))
    return lm, np.array(zs), np.tile([p.vel, p.omega], (STEPS, 1))


def timed(call):
    call()                                     # untimed: captures, allocations
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def main():
    lm, zs, ctl = world()
    rows = []

    def row(name, filters, particles, med, mn, extra=""):
        per_step = med / STEPS
        rows.append(f"{name:<44s} {med:10.3f} {mn:10.3f} {per_step:10.4f} "
                    f"{filters * STEPS / med * 1e3:14.4g} {particles * STEPS / med * 1e3:16.4g}  {extra}")
        print(rows[-1], flush=True)
        return per_step

    a_ms = {}
    for B in (64, 1024, 4096):
        with BatchParticleFilter(B, NP, lm, motion="velocity", seed=np.arange(B) + 1) as e:
            e.load_observations(np.broadcast_to(zs[:, None], (STEPS, B, NL, 2)))
            ev = []

            def call():
                out = e.run(0, ctl)
                ev.append(e.timing()[0])
                return out
            med, mn = timed(call)
            res = call().records
            a_ms[B] = row(f"(a) ensemble B={B}", B, B * NP, med, mn,
                          f"launch {np.median(ev[1:]):.3f} ms, 1 launch, "
                          f"resamples/filter {res['resampled'].sum() / B:.1f}")

    B = 64
    hs = [DeviceParticleFilter(NP, lm, motion="velocity", seed=b + 1) for b in range(B)]
    try:
        for h in hs:
            h.load_observations(zs)
            h.prepare_graphs()

        def call64():
            for h in hs:
                h.run(0, ctl)
        med, mn = timed(call64)
        b_ms = row("(b) 64 DeviceParticleFilter handles in turn", B, B * NP, med, mn)
    finally:
        for h in hs:
            h.close()

    c_ms = {}
    for n in (64000, 1024000):
        with DeviceParticleFilter(n, lm, motion="velocity", seed=1) as d:
            d.load_observations(zs)
            d.prepare_graphs()
            med, mn = timed(lambda: d.run(0, ctl))
            c_ms[n] = row(f"(c) one DeviceParticleFilter NP={n}", 1, n, med, mn)

    head = (f"NP={NP} NL={NL} velocity model, device RNG, product likelihood, {STEPS} steps per run call, "
            f"median / min of {REPS} timed calls after one untimed\n"
            f"{'row':<44s} {'call ms':>10s} {'min ms':>10s} {'ms/step':>10s} {'filter-steps/s':>14s} "
            f"{'particle-steps/s':>16s}")
    tail = [f"(b) / (a) at B=64: {b_ms / a_ms[64]:.1f}x  (ms per ensemble-step {b_ms:.4f} vs {a_ms[64]:.4f})",
            f"(a) B=1024 / (c) NP=1024000: {a_ms[1024] / c_ms[1024000]:.2f}x  "
            f"(ms per step {a_ms[1024]:.4f} vs {c_ms[1024000]:.4f}): 1024 exact per-filter cumsums, "
            "sums and argmaxes against one big filter",
            f"particle-steps/s x NL ({NL}) = particle-observation updates/s in bench.py's sense"]
    text = "\n".join([head] + rows + [""] + tail) + "\n"
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
