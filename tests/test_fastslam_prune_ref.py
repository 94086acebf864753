"""The pruning oracle (tests/fastslam_prune_ref.py) against itself, CPU only:
the vectorised pass against the plain loop, evidence through a resampling,
saturation, removal at the first miss, the empty scan, NaN means, and the claim
of DESIGN 11f -- removal brings the landmark count towards what was observed
and keeps the map from filling."""
import os
import sys

import numpy as np
import pytest

from conftest import ORACLE  # noqa: F401  (puts the oracle on sys.path)

import fastslam2_da_ref as d2
import fastslam_da_ref as da
import fastslam_prune_ref as pr
import fastslam_ref as fr

NOISE = (0.1, np.deg2rad(3.0), np.deg2rad(3.0))
Q = np.diag([0.2, 0.2, np.deg2rad(5.0)]) ** 2


def _filter(parent, n, cap, **kw):
    kw = dict(dict(p_new=0.1, noise=NOISE, ess_th=n / 2.0), **kw)
    if parent == "ml":
        return da.FSDARef(n, cap, **kw)
    return d2.FS2DARef(n, cap, Q, **kw)


def _inputs(parent, rs, n):
    if parent == "ml":
        return rs.multivariate_normal([0.0, 0.0, 0.0], Q, n)
    return rs.standard_normal((n, 3))


def _clone(ref, parent):
    other = _filter(parent, ref.n, ref.cap, p_new=float(np.exp(ref.log_p_new)), ess_th=ref.ess_th)
    other.load(ref)
    other.log_p_new = ref.log_p_new
    return other


# ------------------------------------------------------ vectorised against loop
def _run_both(parent, angle, seed=5):
    """Per step the update by the parent, then the pass twice from the same
    state: vectorised on the filter, the loop on a clone."""
    n, cap, steps = 64, 8, 8
    lm = np.random.RandomState(3).uniform(-12, 12, (7, 2))
    ctl, poses = fr.circle_truth(steps)
    rs = np.random.RandomState(seed)
    cfg = pr.PruneConfig(10.0, view_angle=angle, init=1, hit=1, miss=2, ev_max=3, remove_below=0)
    ref = _filter(parent, n, cap)
    ev = np.zeros((n, cap), dtype=np.int32)
    total = {}
    for pose in poses:
        _, obs = fr.observe(pose, lm, 9.0, NOISE, rs)
        pre = ref.cnt.copy()
        out = ref.step(ctl, obs, _inputs(parent, rs, n), rs.rand() / n)
        if out["resampled"]:
            ev, pre = ev[out["idx"]], pre[out["idx"]]
        twin = _clone(ref, parent)
        ev_v, info = pr.prune_pass(ref, ev, out["assoc"], pre, cfg)
        ev_l, removed = pr.prune_loop(twin, ev, out["assoc"], pre, cfg)
        assert np.array_equal(ev_v, ev_l)
        assert np.array_equal(ref.cnt, twin.cnt)
        assert np.array_equal(info["removed"], removed)
        assert np.array_equal(ref.mean, twin.mean, equal_nan=True)
        assert np.array_equal(ref.cov, twin.cov, equal_nan=True)
        live = np.arange(cap)[None, :] < ref.cnt[:, None]
        assert not np.isnan(ref.mean[live]).any() and np.isnan(ref.mean[~live]).all()
        assert (ev_v[~live] == 0).all()
        for k, v in (("created", (out["assoc"] == da.NEW).sum()), ("matched", (out["assoc"] >= 0).sum()),
                     ("missed", info["in_view"].sum()), ("removed", removed.sum()),
                     ("moved", info["moved"])):
            total[k] = total.get(k, 0) + int(v)
        ev = ev_v
    return total


@pytest.mark.parametrize("parent", ["ml", "ml_marginal"])
@pytest.mark.parametrize("angle", [None, np.deg2rad(80.0)])
def test_vectorised_and_loop_are_bit_equal(parent, angle):
    """NP 64, cap 8, 8 steps of a state that creates, matches, misses, removes
    and moves."""
    seen = _run_both(parent, angle)
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


# ------------------------------------------------------------- single rules
def _set(n, cap, cnt, mean, th=np.pi / 2):
    """A filter at (0, 0, th) holding the given means (covariance identity)."""
    ref = da.FSDARef(n, cap, noise=NOISE, x0=(0.0, 0.0, th))
    ref.cnt = np.asarray(cnt, dtype=np.int32).copy()
    ref.mean = np.full((n, cap, 2), np.nan)
    ref.cov = np.full((n, cap, 3), np.nan)
    for p in range(n):
        ref.mean[p, :ref.cnt[p]] = np.asarray(mean, dtype=np.float64)[:ref.cnt[p]]
        ref.cov[p, :ref.cnt[p]] = (1.0, 0.0, 1.0)
    return ref


def test_evidence_follows_the_particle_through_a_resampling():
    n, cap = 64, 8
    lm = np.random.RandomState(3).uniform(-12, 12, (7, 2))
    ctl, poses = fr.circle_truth(10)
    rs = np.random.RandomState(9)
    flt = pr.PruneRef(_filter("ml", n, cap), pr.PruneConfig(7.2))
    for pose in poses:
        _, obs = fr.observe(pose, lm, 9.0, NOISE, rs)
        flt.step(ctl, obs, _inputs("ml", rs, n), rs.rand() / n)
    # distinct rows, a few heavy particles, then a scan-less step with nothing in view
    flt.ev = (rs.randint(0, 50, (n, cap)) * (flt.ev > 0)).astype(np.int32)
    flt.cfg = pr.PruneConfig(1e-9)
    w = np.full(n, 1e-6)
    w[[3, 17, 40]] = 1.0
    flt.ref.w = w / w.sum()
    ev0, cnt0 = flt.ev.copy(), flt.ref.cnt.copy()
    assert cnt0.max() > cnt0.min() and flt.ref.needs_resample()
    out = flt.step(ctl, np.zeros((0, 3)), _inputs("ml", rs, n), rs.rand() / n)
    idx = out["idx"]
    assert out["resampled"] and set(idx.tolist()) == {3, 17, 40}
    assert not out["in_view"].any() and out["removed"].sum() == 0
    assert np.array_equal(out["cnt0"], cnt0[idx]) and np.array_equal(flt.ref.cnt, cnt0[idx])
    assert np.array_equal(flt.ev, ev0[idx])


def test_saturation_at_ev_max_and_removal_at_the_first_in_view_miss():
    n, cap = 2, 4
    cfg = pr.PruneConfig(5.0, init=1, hit=2, miss=1, ev_max=4, remove_below=1)
    ref = _set(n, cap, [2, 2], [(0.0, 3.0), (0.0, 9.0)])
    ev = np.array([[1, 1, 0, 0], [3, 1, 0, 0]], dtype=np.int32)
    assoc = np.array([[0, 0]], dtype=np.int32)                     # slot 0 matched in both
    ev, info = pr.prune_pass(ref, ev, assoc, ref.cnt.copy(), cfg)
    assert np.array_equal(ev, [[3, 1, 0, 0], [4, 1, 0, 0]])        # 1 + 2; min(3 + 2, 4); out of view
    assert info["removed"].sum() == 0
    # never matched, now in view: remove_below == init removes it at the first miss
    ref.mean[:, 1] = (0.0, 4.0)
    ev, info = pr.prune_pass(ref, ev, np.zeros((0, n), dtype=np.int32), ref.cnt.copy(), cfg)
    assert np.array_equal(info["removed"], [1, 1])
    assert np.array_equal(ref.cnt, [1, 1])
    assert np.array_equal(ev, [[2, 0, 0, 0], [3, 0, 0, 0]])        # slot 0 in view too: -1
    assert np.isnan(ref.mean[:, 1:]).all()


def test_an_empty_scan_decrements_exactly_the_in_view_slots():
    n, cap = 3, 6
    means = [(0.0, 3.0), (6.0, 0.0), (0.0, -3.0), (0.0, 7.3), (5.0, 5.0), (-4.0, 0.1)]
    for angle, inside in ((None, [1, 1, 1, 0, 1, 1]), (np.deg2rad(45.0), [1, 0, 0, 0, 1, 0])):
        cfg = pr.PruneConfig(7.2, view_angle=angle, init=5, miss=2, remove_below=0)
        ref = _set(n, cap, [6, 3, 0], means)
        ev = np.full((n, cap), 5, dtype=np.int32)
        ev2, info = pr.prune_pass(ref, ev, np.zeros((0, n), dtype=np.int32), ref.cnt.copy(), cfg)
        exp = 5 - 2 * np.array(inside)
        assert np.array_equal(ev2[0], exp), angle
        assert np.array_equal(ev2[1], np.r_[exp[:3], 0, 0, 0]), angle
        assert np.array_equal(ev2[2], np.zeros(cap)), angle
        assert info["removed"].sum() == 0 and np.array_equal(ref.cnt, [6, 3, 0])
        twin = _set(n, cap, [6, 3, 0], means)
        ev3, _ = pr.prune_loop(twin, ev, np.zeros((0, n), dtype=np.int32), twin.cnt.copy(), cfg)
        assert np.array_equal(ev2, ev3)


def test_a_nan_mean_is_never_in_view():
    n, cap = 1, 3
    for angle in (None, np.deg2rad(80.0)):
        cfg = pr.PruneConfig(7.2, view_angle=angle, init=1, miss=1, remove_below=1)
        ref = _set(n, cap, [3], [(np.nan, 1.0), (0.0, np.nan), (0.0, 2.0)])
        ev = np.ones((n, cap), dtype=np.int32)
        ev2, info = pr.prune_pass(ref, ev, np.zeros((0, n), dtype=np.int32), ref.cnt.copy(), cfg)
        assert np.array_equal(info["in_view"], [[False, False, True]])
        assert np.array_equal(ev2, [[1, 1, 0]]) and np.array_equal(ref.cnt, [2])
        twin = _set(n, cap, [3], [(np.nan, 1.0), (0.0, np.nan), (0.0, 2.0)])
        ev3, removed = pr.prune_loop(twin, ev, np.zeros((0, n), dtype=np.int32), twin.cnt.copy(), cfg)
        assert np.array_equal(ev2, ev3) and np.array_equal(removed, [1])


# ------------------------------------------------------------------ the claim
def test_removal_brings_the_count_towards_what_was_observed():
    """tools/fastslam_prune_sweep.py's world at NP = 256, seeds 0 to 2,
    evidence +1 / -1, removal below 0, view range 7.2 m (measured: 7 against 15
    at p_new = 0.1, 25 against 87 at 0.3; the inequalities are the test)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "tools"))
    import fastslam_prune_sweep as sw
    n = 256
    for pn in (0.1, 0.3):
        without = [sw.run(n, pn, s) for s in range(3)]
        with_ = [sw.run(n, pn, s, sw.prune_config()) for s in range(3)]
        a, b = sum(r["miss"] for r in without), sum(r["miss"] for r in with_)
        print(f"p_new {pn}: sum |count - observed| {a} without, {b} with; dropped "
              f"{sum(r['dropped'] for r in without)} / {sum(r['dropped'] for r in with_)}")
        assert b < a, (pn, a, b)
        if pn == 0.3:
            assert all(r["dropped"] == 0 for r in with_)
            assert all(r["full"] == n and r["count"] == sw.CAP for r in without)
