"""The fused blocks' partials as one slab (DeferParts: 18 per-block arrays at
slab + j stride, stride a multiple of 16 entries and at least blocks + 1): the
benchmarked path against the oracle (test_gpu_run_oracle.run_lockstep, its
tolerances) at the particle counts where a wrong stride or a wrong pad entry
would show, and the sharded step's reads of the slab against one handle.

Every case: 20 landmarks, 6 steps, ESS_TH = NP / 2 so that a step resamples
(the exact cumsum reads the prefix the step end formed from the slab).
  * 512: one block (stride 16, the pair load of block 0 reads the pad entry);
  * 513: a second block with one valid particle;
  * 1,025: an odd block count (the last pair load's second entry is the pad);
  * 8,192 + 512: one full np.sum buffer (16 leaf entries) plus a tail block;
  * 2^20 + 4,097: the step end's slice pre-pass reads the slab.
"""
import os
import sys

import numpy as np
import pytest

from test_gpu_run_oracle import run_lockstep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

NL, STEPS = 20, 6


@pytest.mark.parametrize("n", [512, 513, 1025, 8192 + 512, (1 << 20) + 4097])
def test_slab_sizes_lockstep_vs_oracle(n):
    run_lockstep(n, NL, STEPS, seed=5, lm_seed=31, obs_seed=32, min_resamples=1, batches=(4, 2),
                 ess_th=n / 2)


def test_slab_one_shard_matches_single():
    """DistFilter(world=1) at 8,192 + 512 particles: the shard path's step end
    (dist_record / dist_finalize) reads the same slab; records and final state
    bit for bit those of one handle on the same seed (bench.compare_to_single)."""
    sys.path.insert(0, ROOT)
    import bench
    import pf_oracle as po
    from slamhip.dist import DistFilter
    from slamhip.pf import DeviceParticleFilter
    n = 8192 + 512
    lm = np.random.RandomState(33).uniform(-10, 10, (NL, 2))
    p = po.PFParams(n_particles=n, landmarks=lm, motion="velocity")
    world = po.PFWorld(p)
    np.random.seed(34)
    zs = []
    for _ in range(STEPS):
        world.advance()
        zs.append(world.observe())
    zs = np.array(zs)
    ctl = np.tile([p.vel, p.omega], (STEPS, 1))
    kw = dict(dt=p.dt, motion="velocity", likelihood="logsum", seed=5, ess_threshold=n / 2)
    single = DeviceParticleFilter(n, lm, **kw)
    dist = DistFilter(n, lm, world=1, **kw)
    try:
        single.load_observations(zs)
        dist.load_observations(zs)
        ra = list(single.run(0, ctl[:4])) + list(single.run(4, ctl[4:]))
        rb = list(dist.run(0, ctl[:4])) + list(dist.run(4, ctl[4:]))
        assert sum(bool(r["resampled"]) for r in ra) >= 1
        ok, worst, first = bench.compare_to_single(rb, dist.get_state(), ra, single.get_state())
        assert ok, (first, worst)
    finally:
        dist.close()
        single.close()
