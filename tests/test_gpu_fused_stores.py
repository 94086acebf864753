"""The deferred fused tile's pair stores (x, y, th of the predicted pair and
w_un in place, 16 bytes per lane; write-through on handles of this size) at
the smallest sizes at which they can go wrong, against the oracle.

The yardstick is test_gpu_run_oracle.run_lockstep: every step of the benchmarked
path (slam_pf_run, device noise) against PFOracle.step on the device's own
normals -- particles, weights, np.sum, argmax, ESS, cov -- reading the state
back after every step, then the same steps in multi-step graph batches bit for
bit against the one-step batches.

  n        what it exercises
  512      one full block
  513      a second block holding one valid particle, and a lane whose pair
           straddles n and is stored into the padding
  1,023    odd n, two blocks
  4,601    ragged, ten blocks
  66,049   more blocks than one CU round of an XCD holds (130 blocks)

20 landmarks, 10 steps, ESS_TH = n / 10, batches (4, 3, 2, 1).  With these the
oracle's ESS / n falls 0.42, 0.17, 0.06 from a resample on (the same at every
size to two digits), so steps 3, 6 and 9 resample -- two of them inside a
multi-step graph, on alternate ones the direct index form -- and seven do
not; each case asserts at least two of either kind from the printed counts.

The other deferred instantiations of the tile at n = 4,601: the product
likelihood on the same path, and the host-noise step() path in both likelihood
modes, checked as tests/test_gpu_c2.py checks C2 (its run_lockstep, its
tolerances) on a trajectory of the oracle at this size.
"""
import re

import numpy as np
import pytest

import pf_oracle as po
import test_gpu_c2
import test_gpu_run_oracle as tro

pytestmark = pytest.mark.gpu

NL, STEPS, BATCHES = 20, 10, (4, 3, 2, 1)
SIZES = (512, 513, 1023, 4601, 66049)


def _lockstep_counted(capsys, n, seed):
    inside = tro.run_lockstep(n, NL, STEPS, seed=seed, lm_seed=31, obs_seed=32, min_resamples=2,
                              batches=BATCHES, ess_th=n / 10)
    out = capsys.readouterr().out
    kinds = [m.group(1) in ("1", "True") for m in re.finditer(r"^step \d+: resampled (\S+)", out, re.M)]
    n_res, n_idle = sum(kinds), len(kinds) - sum(kinds)
    with capsys.disabled():
        print(out, end="")
        print(f"n={n}: {n_res} resampling steps ({inside} inside a multi-step graph), "
              f"{n_idle} non-resampling steps")
    assert len(kinds) == STEPS
    assert n_res >= 2 and n_idle >= 2, (n_res, n_idle)
    assert inside >= 1, inside


@pytest.mark.parametrize("n", SIZES)
def test_pair_stores_lockstep_vs_oracle(capsys, n):
    _lockstep_counted(capsys, n, seed=5)


def test_pair_stores_product_likelihood(capsys, monkeypatch):
    """pf_fused_kernel<velocity, product, device noise, deferred>: the same
    lockstep with the handles in the reference-literal product mode."""
    def handle(p, seed):
        from slamhip.pf import DeviceParticleFilter
        return DeviceParticleFilter(p.np, p.lm, dt=p.dt, motion="velocity", likelihood="product",
                                    alphas=p.alphas, seed=seed, ess_threshold=p.ess_th)
    monkeypatch.setattr(tro, "_handle", handle)
    _lockstep_counted(capsys, 4601, seed=6)


@pytest.fixture(scope="module")
def trajectory_4601():
    """The oracle's trajectory at n = 4,601 in the form of conftest.c2_trajectory
    (host-injected normals and offsets), computed once for both modes."""
    n = 4601
    rs = np.random.RandomState(33)
    lm = rs.uniform(-10, 10, (NL, 2))
    p = po.PFParams(n_particles=n, landmarks=lm, motion="velocity")
    p.ess_th = n / 10
    orc, world = po.PFOracle(p), po.PFWorld(p)
    np.random.seed(34)
    steps = []
    for _ in range(STEPS):
        world.advance()
        state = (orc.x.copy(), orc.y.copy(), orc.th.copy(), orc.w.copy())
        u = np.random.rand() if orc.needs_resample() else None
        g = np.random.standard_normal(3 * n).reshape(n, 3)
        z = world.observe()
        out = orc.step(z, g, None if u is None else u * p.np_recip)
        steps.append(dict(state=state, u=u, g=g, z=z, out=out,
                          post=(orc.x.copy(), orc.y.copy(), orc.th.copy(), orc.w.copy()),
                          resample_next=orc.needs_resample()))
    n_res = sum(bool(s["out"]["resampled"]) for s in steps)
    print(f"n={n} host-noise trajectory: {n_res} resampling steps, {STEPS - n_res} others")
    assert n_res >= 2 and STEPS - n_res >= 2, n_res
    return p, steps


@pytest.mark.parametrize("lik", ["logsum", "product"])
def test_pair_stores_host_noise_step(trajectory_4601, monkeypatch, lik):
    """pf_fused_kernel<velocity, lik, host noise, deferred> through step():
    test_gpu_c2's lockstep on the n = 4,601 trajectory (its device is built for
    C2's size and default threshold, so only the constructor is replaced)."""
    def dev(p, lik):
        from slamhip.pf import DeviceParticleFilter
        return DeviceParticleFilter(p.np, p.lm, dt=p.dt, motion="velocity", likelihood=lik,
                                    alphas=p.alphas, ess_threshold=p.ess_th)
    monkeypatch.setattr(test_gpu_c2, "_dev", dev)
    test_gpu_c2.run_lockstep(trajectory_4601, lik)
