"""The split step end of device-resident batches (pf_finalize.inl, NP <= 2^20)
against the full one, bit for bit.

Inside a batch, before its last step, finalize_fast_kernel<false> runs as a
few independent workgroups: workgroup 0 ends the step without the covariance
moments, the moment workgroups store their raw totals, and slam_pf_run forms
the records' cov on the host.  A batch's last step takes the full path, which
is the code every step took before the split.

Two handles with the same seed, landmarks, observations and controls run the
same 13 steps: handle A as batches of 5 and 8 steps (graphs of 4 + 1 and 8
steps: all but two step ends are split), handle B as 13 batches of one step
(every step end full).  Every field of every record and the final state must
be equal bit for bit (NaN equal to NaN).  No tolerance: the split reduces each
quantity in the full path's order, and host and device form cov by one
expression without contraction.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NL, STEPS, SPLIT_AT = 20, 13, 5
DT = 0.1
OMEGA = np.deg2rad(10.0)
VEL = 10.0 * OMEGA
# the fraction of NP below which the ESS triggers a resample (the default is
# NP / 100).  One update from uniform weights leaves the ESS near 0.45 NP with
# these 20 landmarks and a second one near 0.15 NP, at every size below: NP / 2
# would resample at every step, 0.3 NP resamples at every other one
ESS_FRAC = 0.3


def _world(seed=7):
    """Landmarks and their robot-frame observations along the noise-free
    velocity trajectory from the filter's start pose (motion_model.py:64-86,
    particle_filter.py:144-154), as bench.simulate_world forms them."""
    from mylib import limit
    from mylib import transform as tf
    rs = np.random.RandomState(seed)
    lm = rs.uniform(-10.0, 10.0, (NL, 2))
    r = np.diag([0.3, 0.3]) ** 2
    x = np.array([[10.0], [0.0], [np.pi / 2]])
    zs = np.empty((STEPS, NL, 2))
    for k in range(STEPS):
        a = VEL / OMEGA
        y2 = limit.limit_angle(x[2, 0] + limit.limit_angle(OMEGA * DT))
        x = np.array([[x[0, 0] + a * (-np.sin(x[2, 0]) + np.sin(y2))],
                      [x[1, 0] + a * (np.cos(x[2, 0]) - np.cos(y2))], [y2]])
        zs[k] = tf.world2robot(x, lm) + rs.multivariate_normal([0.0, 0.0], r, NL)
    return lm, zs


def _filter(n, lm, zs):
    from slamhip.pf import DeviceParticleFilter
    pf = DeviceParticleFilter(n, lm, dt=DT, motion="velocity", likelihood="logsum", seed=4321,
                              ess_threshold=ESS_FRAC * n)
    pf.load_observations(zs)
    return pf


def _run_both(n, zs_edit=None):
    """(records of handle A, of handle B, state of A, state of B)"""
    lm, zs = _world()
    if zs_edit is not None:
        zs_edit(zs)
    ctl = np.tile([VEL, OMEGA], (STEPS, 1))
    a, b = _filter(n, lm, zs), _filter(n, lm, zs)
    try:
        ra = np.concatenate([a.run(0, ctl[:SPLIT_AT]).records.copy(),
                             a.run(SPLIT_AT, ctl[SPLIT_AT:]).records.copy()])
        rb = np.concatenate([b.run(k, ctl[k:k + 1]).records.copy() for k in range(STEPS)])
        return ra, rb, a.get_state(), b.get_state()
    finally:
        a.close()
        b.close()


def _assert_equal(ra, rb, sa, sb):
    assert ra.dtype == rb.dtype and len(ra) == len(rb) == STEPS
    for name in ra.dtype.names:
        x, y = ra[name], rb[name]
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (name, x, y)
    for x, y in zip(sa, sb):
        assert np.array_equal(x, y, equal_nan=True)


# 512: one fused block (only lane 0 holds one; np.sum takes the tail path only)
# 1,000: a ragged second block (a pair load with one valid half)
# 12,345: one full 8192 buffer plus a tail; 25 blocks, an odd count
# 524,800: 1,025 blocks -- the first block of the second register half, fin_blk(0, 2)
# 1,048,576: all 2,048 blocks (the bench's shape)
@pytest.mark.parametrize("n", [512, 1000, 12345, 524800, 1 << 20])
def test_split_step_end_matches_full(n):
    ra, rb, sa, sb = _run_both(n)
    print(f"NP {n}: resampled {ra['resampled'].tolist()} ess/NP "
          f"{np.round(ra['ess'] / n, 3).tolist()}")
    _assert_equal(ra, rb, sa, sb)
    assert np.all(np.isfinite(ra["cov"]))
    # both kinds of step, or the run checked one path of the step end only
    assert int(np.sum(ra["resampled"] == 1)) >= 2, ra["resampled"]
    assert int(np.sum(ra["resampled"] == 0)) >= 2, ra["resampled"]


def test_degenerate_step_inside_a_batch():
    """Step 7, inside handle A's 8-step batch, sees observations that make
    every likelihood zero: workgroup 0 takes the ok == false path (every
    moment from the normalised weights, the entry marked complete); that
    record and the later ones must still equal the full path's."""
    bad = 7

    def edit(zs):
        zs[bad] = 1e3

    ra, rb, sa, sb = _run_both(12345, edit)
    ws = ra["weight_sum"][bad]
    print(f"degenerate step {bad}: weight_sum {ws!r}, resampled {ra['resampled'].tolist()}")
    assert not (ws > 0.0) or not np.isfinite(ws), ws
    _assert_equal(ra, rb, sa, sb)
