"""The landmark map on the GPU against the NumPy restatement
tests/graph_map_ref.py.

Shapes: random poses, one to five landmarks, per-landmark counts 0, 1, 2, W - 1,
W, W + 1, 2W + 1 (W = 256, the fold's chunk) and one landmark with 5000, the
half-edges of different landmarks interleaved at random, some with ids outside
[0, n_landmarks).

Bars (the convention of test_gpu_graph_robust.py): mean within 1e-12 m, cov
within 1e-12 of its largest entry, chi2_k and chi2_l within 1e-11 max(1, chi2).
The restatement's own rounding is far below them (float64 against longdouble,
sequentially and in a 256-wide tree, n from 1 to 5000: <= 8e-16 m and <= 5e-16
relative).  The end-to-end means are held to 1e-8, the bar
test_t300_gauss_newton_loop_matches_reference uses for the poses they are
evaluated at.  Measured on the device: DESIGN 8.7.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import graph_map_ref as mr
import graph_odom_ref as gr

pytestmark = pytest.mark.gpu

W = 256
N_POSES = 40


def _dev(**kw):
    from slamhip.graph import DeviceGraph
    kw.setdefault("solver", "dense")
    return DeviceGraph(**kw)


@functools.lru_cache(maxsize=None)
def _poses():
    rs = np.random.RandomState(11)
    p = np.column_stack([rs.uniform(-10, 10, N_POSES), rs.uniform(-10, 10, N_POSES),
                         rs.uniform(-np.pi, np.pi, N_POSES)])
    p.setflags(write=False)
    return p


def _rows(rs, landmark, n):
    """n half-edge rows of one landmark id from random poses."""
    p = rs.randint(0, N_POSES, n)
    return np.column_stack([p, p, np.full(n, landmark), rs.uniform(2, 15, n), rs.uniform(-np.pi, np.pi, n),
                            rs.uniform(-np.pi, np.pi, n)]).astype(np.float64).reshape(n, 6)


def _interleave(rs, groups):
    """Rows of several landmarks shuffled together, each landmark's own order kept."""
    tag = rs.permutation(np.repeat(np.arange(len(groups)), [len(g) for g in groups]))
    nxt = [0] * len(groups)
    out = np.empty((len(tag), 6))
    for i, g in enumerate(tag):
        out[i] = groups[g][nxt[g]]
        nxt[g] += 1
    return out


CASES = {"small": (5, (0, 1, 2, W - 1, W)), "large": (3, (W + 1, 2 * W + 1, 5000)), "one": (1, (W + 1,)),
         "single": (1, (1,))}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(halves, n_landmarks, the restatement's map): computed once, read-only."""
    nl, counts = CASES[name]
    rs = np.random.RandomState(sorted(CASES).index(name))
    groups = [_rows(rs, l, n) for l, n in enumerate(counts)]
    if name == "small":
        groups += [_rows(rs, nl, 3), _rows(rs, -1, 2)]            # ignored ids on both sides
    halves = _interleave(rs, groups)
    ref = mr.landmark_map(halves, nl, _poses())
    for a in (halves,) + ref:
        a.setflags(write=False)
    return halves, nl, ref


def _close(name, got, want, bar):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), name
    ok = ~np.isnan(want)
    diff = np.abs(got[ok] - want[ok]) / np.broadcast_to(bar, want.shape)[ok]
    worst = float(diff.max()) if diff.size else 0.0
    print("%s: worst difference %.3g of its bar" % (name, worst))
    assert worst <= 1.0, (name, worst)


# ------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_restatement(name):
    halves, nl, (mean, cov, count, chi2, half) = _case(name)
    dev = _dev()
    try:
        dev.set_poses(_poses())
        dev.set_observations(halves, nl)
        dmean, dcov, dcount, dchi2, dhalf = dev.landmarks(per_observation=True)
        np.testing.assert_array_equal(dcount, count)
        assert sorted(count.tolist()) == sorted(CASES[name][1])
        _close(name + " mean", dmean, mean, 1e-12)
        big = np.nanmax(np.abs(cov).reshape(nl, 4), axis=1) if nl else np.empty(0)
        _close(name + " cov", dcov, cov, 1e-12 * np.where(np.isnan(big), 1.0, big)[:, None, None])
        _close(name + " chi2_l", dchi2, chi2, 1e-11 * np.maximum(1.0, np.nan_to_num(chi2)))
        _close(name + " chi2_k", dhalf, half, 1e-11 * np.maximum(1.0, np.nan_to_num(half)))
        np.testing.assert_array_equal(dcov[:, 0, 1], dcov[:, 1, 0])
        # the per-landmark sums are those of the device's own per-observation values
        ids = halves[:, 2].astype(np.int64)
        for l in np.flatnonzero(count):
            np.testing.assert_allclose(dchi2[l], dhalf[ids == l].sum(), rtol=1e-12)
        # without the per-observation output the same bits
        for u, v in zip(dev.landmarks(), (dmean, dcov, dcount, dchi2)):
            np.testing.assert_array_equal(u, v)
        t = dev.map_timing()
        assert t["launches"] == 5 and t["ms"] > 0
    finally:
        dev.close()


def test_exact_cases():
    """n_l = 1: mean = L_k and chi2 = 0 exactly; ignored ids: NaN in half_chi2;
    a landmark nobody saw: NaN; half_chi2 in input order."""
    halves, nl, (mean, _, count, _, half) = _case("small")
    dev = _dev()
    try:
        dev.set_poses(_poses())
        dev.set_observations(halves, nl)
        dmean, dcov, dcount, dchi2, dhalf = dev.landmarks(per_observation=True)
        ids = halves[:, 2].astype(np.int64)
        ignored = (ids < 0) | (ids >= nl)
        assert ignored.sum() == 5 and np.isnan(dhalf[ignored]).all() and not np.isnan(dhalf[~ignored]).any()
        (l1,) = np.flatnonzero(count == 1)
        (k1,) = np.flatnonzero(ids == l1)
        assert dchi2[l1] == 0.0 and dhalf[k1] == 0.0
        L, C, _ = mr.half_terms(halves[k1], _poses())
        np.testing.assert_allclose(dmean[l1], L, rtol=0, atol=1.5e-14)  # sincos against NumPy's: ulps of 32 m
        np.testing.assert_allclose(dcov[l1], C, rtol=0, atol=1e-12 * np.abs(C).max())
        # mean = L_k exactly, as the device places it: a second landmark holding the same
        # observation twice has mean = L_k too (eta = 0 exactly)
        twice = np.concatenate([halves[k1:k1 + 1]] * 2)
        twice[:, 2] = 0
        dev.set_observations(twice, 1)
        m2, _, c2, x2, h2 = dev.landmarks(per_observation=True)
        np.testing.assert_array_equal(m2[0], dmean[l1])
        assert c2[0] == 2 and x2[0] == 0.0 and not h2.any()
        (l0,) = np.flatnonzero(count == 0)
        assert np.isnan(dmean[l0]).all() and np.isnan(dcov[l0]).all() and np.isnan(dchi2[l0])
    finally:
        dev.close()


def test_no_half_edges_clears_the_observations():
    dev = _dev()
    try:
        dev.set_poses(_poses())
        dev.set_observations(_case("single")[0], 1)
        dev.landmarks()
        dev.set_observations(np.empty((0, 6)), 3)
        with pytest.raises(RuntimeError, match="no observations"):
            dev.landmarks()
        # every half-edge ignored, and no landmark at all: empty and NaN, no launch needed
        dev.set_observations(_case("single")[0], 0)
        mean, cov, count, chi2, half = dev.landmarks(per_observation=True)
        assert mean.shape == (0, 2) and cov.shape == (0, 2, 2) and len(count) == len(chi2) == 0
        assert np.isnan(half).all() and len(half) == 1
        assert dev.map_timing()["launches"] == 0
    finally:
        dev.close()


# ------------------------------------------------------------ 2. determinism
def test_bit_identical_from_call_to_call():
    halves, nl, _ = _case("large")
    dev = _dev()
    try:
        dev.set_poses(_poses())
        dev.set_observations(halves, nl)
        a = dev.landmarks(per_observation=True)
        b = dev.landmarks(per_observation=True)
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)
    finally:
        dev.close()


@pytest.mark.parametrize("n", [2 * W + 1, 5000])
def test_a_landmark_does_not_depend_on_the_others(n):
    """The same half-edges of one landmark, alone as landmark 0 and as landmark 2
    among others interleaved two ways: mean, cov, chi2 and its chi2_k bit for bit."""
    rs = np.random.RandomState(n)
    own = _rows(rs, 0, n)
    dev = _dev()
    try:
        dev.set_poses(_poses())
        dev.set_observations(own, 1)
        mean, cov, count, chi2, half = dev.landmarks(per_observation=True)
        assert count[0] == n
        moved = own.copy()
        moved[:, 2] = 2
        for others in ([_rows(rs, 0, 700), _rows(rs, 1, 3), _rows(rs, 3, W)],
                       [_rows(rs, 3, 5), _rows(rs, 9, 40), _rows(rs, 0, 1)]):
            mixed = _interleave(rs, [moved] + others)
            dev.set_observations(mixed, 4)
            m2, c2, n2, x2, h2 = dev.landmarks(per_observation=True)
            assert n2[2] == n
            np.testing.assert_array_equal(m2[2], mean[0])
            np.testing.assert_array_equal(c2[2], cov[0])
            assert x2[2] == chi2[0]
            np.testing.assert_array_equal(h2[mixed[:, 2] == 2], half)      # and in input order
    finally:
        dev.close()


# ------------------------------------------------------- 3. argument errors
def test_record_errors_leave_the_handle_as_it_was():
    from slamhip import _lib
    halves, nl, _ = _case("small")
    dev = _dev()
    try:
        dev.set_poses(_poses())
        dev.set_observations(halves, nl)
        before = dev.landmarks(per_observation=True)
        for col, val, msg in ((1, N_POSES, "pose index"), (1, -1, "pose index"), (3, np.nan, "not finite"),
                              (4, np.inf, "not finite"), (5, np.nan, "not finite"), (3, 0.0, "distance"),
                              (3, -1.0, "distance")):
            bad = halves[:7].copy()
            bad[5, col] = val
            with pytest.raises(RuntimeError, match=msg):
                dev.set_observations(bad, nl)
            for u, v in zip(dev.landmarks(per_observation=True), before):
                np.testing.assert_array_equal(u, v)
        # another pose count drops them
        dev.set_poses(_poses()[:N_POSES - 1])
        with pytest.raises(RuntimeError, match="no observations"):
            dev.landmarks()
        # members drop them, and a handle with members takes none
        dev.set_poses(_poses())
        dev.set_observations(halves, nl)
        off = np.array([0, 20, N_POSES], dtype=np.int64)
        _lib.check(dev._lib.slam_graph_set_members(dev._h, 2, off.ctypes.data_as(C.POINTER(C.c_int64))),
                   "slam_graph_set_members")
        with pytest.raises(RuntimeError, match="no observations"):
            dev.landmarks()
        with pytest.raises(RuntimeError, match="members"):
            dev.set_observations(halves, nl)
    finally:
        dev.close()


# -------------------------------------------------------- 4. non-interference
def _world_handle(observe):
    from slamhip.graph import edge_array
    w = mr.world(5)
    dev = _dev()
    dev.set_poses(w["start"])
    dev.set_edges(edge_array(w["edges"]), odometry=w["odom"])
    if observe:
        dev.set_observations(w["halves"], 16)
    return dev, w


def test_landmarks_between_updates_changes_nothing():
    plain, w = _world_handle(False)
    obs, _ = _world_handle(True)
    try:
        for _ in range(3):
            obs.landmarks(per_observation=True)
            assert plain.update() == obs.update()
            obs.landmarks()
            np.testing.assert_array_equal(plain.get_poses(), obs.get_poses())
            for u, v in zip(plain.get_system(dense=True, blocks=True), obs.get_system(dense=True, blocks=True)):
                np.testing.assert_array_equal(u, v)
            np.testing.assert_array_equal(plain.get_delta(), obs.get_delta())
            assert plain.chi2() == obs.chi2()
        # set_poses of the same count keeps the observations; the map sees the new poses
        obs.set_poses(w["truth"])
        mean, cov, count, chi2 = obs.landmarks()
        rmean, rcov, rcount, rchi2, _ = mr.landmark_map(w["halves"], 16, w["truth"])
        np.testing.assert_array_equal(count, rcount)
        _close("truth mean", mean, rmean, 1e-12)
        _close("truth chi2", chi2, rchi2, 1e-11 * np.maximum(1.0, rchi2))
    finally:
        plain.close()
        obs.close()


# ------------------------------------------------------------- 5. end to end
def test_estimator_map_matches_restatement():
    """Seed 5, 72 poses, 16 landmarks: the device loop with odometry through
    TrajectoryEstimator, then getEstLandMarks, against the restatement's map at
    the restatement's optimised poses."""
    from graph_based_slam import HalfEdge, Observation, TrajectoryEstimator
    w = mr.world(5)
    te = TrajectoryEstimator(w["start"][0].reshape(3, 1).copy(), solver="dense")
    assert te.getEstLandMarks() is None
    te.setOdometry(gr.SIGMA)
    for k in range(1, 72):
        te.addPose(w["start"][k].reshape(3, 1).copy(), True, w["odom"]["rel"][k - 1])
    halves = [HalfEdge(int(r[0]), Observation(int(r[2]), r[3], r[4], r[5]), int(r[1])) for r in w["halves"]]
    st = te.estimate_trajectory(halves, 16)
    assert bool(st[-1][0])
    est = te.getEstLandMarks()
    ref_poses = mr.cpu_optimised(5)
    np.testing.assert_allclose(np.array([p[:, 0] for p in te._poses]), ref_poses, rtol=0, atol=1e-8)
    rmean, rcov, rcount, rchi2, _ = mr.landmark_map(w["halves"], 16, ref_poses)
    assert sorted(est) == np.flatnonzero(rcount).tolist() == list(range(16))
    mean = np.array([est[l][0] for l in range(16)])
    worst = np.abs(mean - rmean).max()
    print("end to end: worst mean difference %.3g m" % worst)
    assert worst <= 1e-8
    for l in range(16):
        assert est[l][1].shape == (2, 2) and est[l][2] == rcount[l]
        np.testing.assert_allclose(est[l][3], rchi2[l], rtol=1e-5, atol=1e-6)
    rms = mr.map_rms(mean, w["landmarks"])
    rms_start = mr.map_rms(mr.landmark_map(w["halves"], 16, w["start"])[0], w["landmarks"])
    print("end to end: map RMS %.3f m, dead-reckoned %.3f m" % (rms, rms_start))
    assert rms < rms_start


def test_robot_returns_and_draws_its_map():
    """The demo's robot with odometry edges: getEstLandMarks after the estimate
    is closer to the true landmarks than the map of the dead-reckoned poses, and
    the world frame draws with the estimated landmarks on an Agg canvas."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import graph_based_slam as gs
    np.random.seed(7)
    x0 = np.array([[10.0], [0.0], [np.deg2rad(90.0)]])
    rbt = gs.Robot(x0, gs.PERIOD_ms / 1000, gs.SCN_SENS_RANGE_m, gs.SCN_SENS_ANGLE_rps, gs.LAND_MARKS)
    rbt.setOdometry((0.02, 0.02, 0.01))
    assert rbt.getEstLandMarks() is None
    for _ in range(18):
        rbt.move(gs.VEL_mps, gs.OMEGA_rps)
    dead = np.array([p[:, 0] for p in rbt._est._poses])
    st = rbt.estimateOpticalTrajectory()
    assert bool(st[-1][0])
    est = rbt.getEstLandMarks()
    assert est and all(0 <= l < len(gs.LAND_MARKS) for l in est)
    ids = sorted(est)
    mean = np.array([est[l][0] for l in ids])
    # the same observations at the dead-reckoned poses
    dev = rbt._est._dev
    opt = dev.get_poses()
    dev.set_poses(dead)
    mean0 = dev.landmarks()[0][ids]
    dev.set_poses(opt)
    rms = np.sqrt(np.mean(np.sum((mean - gs.LAND_MARKS[ids]) ** 2, axis=1)))
    rms0 = np.sqrt(np.mean(np.sum((mean0 - gs.LAND_MARKS[ids]) ** 2, axis=1)))
    print("robot: %d landmarks, map RMS %.3f m, dead-reckoned %.3f m" % (len(ids), rms, rms0))
    assert rms < rms0
    for l in ids:
        m, cov, n, chi2 = est[l]
        assert m.shape == (2,) and cov.shape == (2, 2) and n >= 1 and chi2 >= 0.0
        assert np.all(np.linalg.eigvalsh(0.5 * (cov + cov.T)) > 0)
    fig, (ax1, ax2) = plt.subplots(1, 2)
    try:
        rbt.draw(ax1, ax2)
        n_before = len(ax1.patches)
        rbt.drawEstLandMarks(ax1)
        assert len(ax1.patches) == n_before + len(ids)
        fig.canvas.draw()
    finally:
        plt.close(fig)
