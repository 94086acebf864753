"""The merged exact-cumsum launch's hand-off: what its last block
hands to the waiting blocks travels as tagged 8-byte granules {payload, epoch}
-- each block's global offsets in a record of its own, the folded specials,
the fold's verdict -- with no fence on either side.  What can go wrong there shows at
small sizes: two or more blocks, a partial last tile, waves without a tile,
specials in tiles that are not the first of their block (read through their
tags, not from the record), heavy elements that own many fused blocks (the
carry path), and -- the failure mode tags add -- a record or special of an
EARLIER launch that is taken for this launch's.

The oracle is particle_filter.py:212-221 as oracle/pf_oracle.py restates it
(np.cumsum + searchsorted); indices are compared bit for bit, so there is no
tolerance anywhere in this file.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SIZES = [2049, 4097, 3 * 2048 + 1, 65536 + 513]
N_RUN = 65536 + 513


def handoff_weights(n, seed, doublings=10):
    """A leading run of exact zeros that ends inside the SECOND tile of the
    first block; then, at two places that are not in the first tile of their
    block, `doublings` elements that each double the running sum (a binade
    crossing each: specials) followed by an element 0.8 times everything before
    it; a last element (the partial tile) of half the rest.  The second place's
    heavy element and the last one hold about 0.3 of the mass each: more than
    512 positions for every n here.  Small weights elsewhere."""
    rs = np.random.RandomState(seed)
    w = rs.random_sample(n) * 1e-12
    w[:700] = 0.0
    for p in (700, n // 2 + 600):
        assert p % 2048 >= 512 and p + doublings + 1 < n
        run = float(np.sum(w[:p]))
        for i in range(doublings):
            w[p + i] = max(run, 1e-12) * 1.5
            run += w[p + i]
        w[p + doublings] = 0.8 * run
    w[n - 1] = 0.5 * float(np.sum(w[:n - 1]))
    return w / np.sum(w.reshape(1, n))


@pytest.mark.parametrize("n", SIZES)
def test_indices_exact_merged_and_two_launch(n):
    import pf_oracle as po
    from slamhip import pf as dpf
    w = handoff_weights(n, n % 9973)
    u = 0.37
    ref = po.systematic_indices(w, u * (1.0 / n))
    assert np.all(ref >= 0)
    # the heavy elements own more than one fused block (512 positions) each
    assert np.max(np.bincount(ref, minlength=n)) > 512
    for merged in (True, False):
        with dpf.DeviceParticleFilter(n, np.zeros((1, 2))) as d:
            d.set_scan_merged(merged)
            d.set_state(w=w)
            idx, nspec = d.resample_indices(u)
        print(f"n={n} merged={merged} n_special={nspec}")
        np.testing.assert_array_equal(idx, ref, err_msg=f"merged={merged}")
        assert nspec >= 2, nspec


@pytest.mark.parametrize("n", [4097, 65536 + 513])
def test_consecutive_launches_do_not_read_stale_records(n):
    """One handle, five exact cumsums in a row with different weights and
    offsets; the special count falls at least once from one call to the next,
    so that the earlier call's surplus specials (and every block's earlier
    record) are still in memory with their old tags."""
    import pf_oracle as po
    from slamhip import pf as dpf
    calls = [(24, 0.11), (40, 0.83), (3, 0.52), (30, 0.29), (6, 0.71)]
    counts = []
    with dpf.DeviceParticleFilter(n, np.zeros((1, 2))) as d:
        d.set_scan_merged(True)
        for k, (doublings, u) in enumerate(calls):
            w = handoff_weights(n, 100 + k, doublings)
            ref = po.systematic_indices(w, u * (1.0 / n))
            d.set_state(w=w)
            idx, nspec = d.resample_indices(u)
            np.testing.assert_array_equal(idx, ref, err_msg=f"call {k}")
            counts.append(nspec)
    print(f"n={n} n_special per call: {counts}")
    assert min(counts) >= 2
    assert any(b < a for a, b in zip(counts, counts[1:])), counts


def run_path(merged, n=N_RUN, steps=12):
    """Twelve device-decided steps (marks only, hipGraph batches) in two
    batches, every step after the first resampling: records and final state."""
    import bench
    from slamhip import pf as dpf
    lm, zs, (vel, omega, dt) = bench.simulate_world(steps)
    ctl = np.tile([vel, omega], (steps, 1))
    with dpf.DeviceParticleFilter(n, lm, dt=dt, motion="velocity", likelihood="logsum", seed=3,
                                  ess_threshold=float(n) + 1.0) as d:
        d.set_scan_merged(merged)
        d.load_observations(zs)
        recs = list(d.run(0, ctl[:5])) + list(d.run(5, ctl[5:]))
        state = d.get_state()
    return recs, state


def same_run(a, b):
    for k, (p, q) in enumerate(zip(a[0], b[0])):
        for f in ("resampled", "resample_next", "max_idx", "max_val", "weight_sum", "ess", "status",
                  "n_special"):
            assert p[f] == q[f], (k, f, p[f], q[f])
        np.testing.assert_array_equal(p["x_est"], q["x_est"], err_msg=f"step {k}")
        np.testing.assert_array_equal(p["cov"], q["cov"], err_msg=f"step {k}")
    for u, v in zip(a[1], b[1]):
        np.testing.assert_array_equal(u, v)


def clean(run):
    recs = run[0]
    assert sum(int(r["resampled"]) for r in recs) >= len(recs) - 1
    bad = [(k, r["status"]) for k, r in enumerate(recs) if r["status"] & (2 | 8)]
    assert not bad, f"fallback (2) / bounded wait (8) at {bad}"


@pytest.fixture(scope="module")
def merged_run():
    return run_path(True)


def test_run_path_merged_matches_two_launch(merged_run):
    clean(merged_run)
    two = run_path(False)
    clean(two)
    same_run(merged_run, two)


def test_handoff_under_a_second_process(merged_run):
    """Uneven load: a second process runs the same small filter on the same
    GPU while this one repeats the run; both must reproduce the quiet run and
    no block may give up waiting."""
    peer = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--peer", "4"],
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    try:
        line = peer.stdout.readline()                 # the peer has the GPU open and has run once
        assert line.strip() == "ready", (line, peer.stderr.read() if peer.poll() is not None else "")
        for _ in range(3):
            r = run_path(True)
            clean(r)
            same_run(merged_run, r)
        out, err = peer.communicate(timeout=120)
    finally:
        if peer.poll() is None:
            peer.kill()
    assert peer.returncode == 0, err[-2000:]
    assert "peer ok" in out, out


def _peer(reps):
    for p in (os.path.join(ROOT, "slam-robot_simu_amd"), os.path.join(ROOT, "oracle"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    first = run_path(True)
    clean(first)
    print("ready", flush=True)
    for _ in range(reps):
        r = run_path(True)
        clean(r)
        same_run(first, r)
    print("peer ok", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--peer":
        _peer(int(sys.argv[2]))
