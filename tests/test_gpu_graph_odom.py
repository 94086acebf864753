"""Odometry edges on the GPU against the NumPy restatement
tests/graph_odom_ref.py.

The base case is circle_graph(72, n_landmarks=16, seed=5) with its 71 odometry
edges: E_lm = 264, so the boundary between the two kinds of column falls inside
a wave and inside a chi-square workgroup.  The pair list is also truncated to
E_lm in {0, 1, 100, 128, 256}, and the odometry list to 1 edge.

Tolerances are those of test_gpu_graph_robust.py for the same quantities: H atol
1e-12 max|H|, b atol 1e-11 max|b|; chi2_e rtol 1e-9, atol 1e-12 (err carries
~2e-15 of absolute rounding and Omega <= 1e4: a relative error of 2e-15 / |err|,
below 1e-9 for |err| > 2e-6, and under 1e-16 absolute below that); w_e rtol
2e-9 on the landmark columns and exactly 1 on the odometry ones; the totals
against the sums of the device's own per-edge arrays rtol 1e-12, bit-identical
from call to call.  An odometry column's 36 H values are summands of H and take
H's form, atol 1e-12 max|column|; its 6 b values atol 1e-11 max|column's b|.
delta is compared in every case (all are solved, cond(H) <= 2.6e7), to cond(H) *
1e-12 * max|delta|: the H and b tolerances carried through the solve.  The
marginal covariance of an unobserved pose: the dense bar of
test_gpu_graph_marginals.py, max(1e-11 max|Sigma|, 64 spread).  Final poses of
the Gauss-Newton loop: atol 1e-8, the bar of
test_t300_gauss_newton_loop_matches_reference.
"""
import ctypes as C
import os

import numpy as np
import pytest

import graph_odom_ref as gr
import graph_robust_ref as rr

pytestmark = pytest.mark.gpu

KINDS = [(None, None), ("huber", 1.0), ("cauchy", 2.0), ("dcs", 5.0)]
E_LM = [0, 1, 100, 128, 256, 264]
E_OD = [1, 71]


def _name(kind, k):
    return "none" if kind is None else "%s%g" % (kind, k)


def _dev(robust=None, **kw):
    from slamhip.graph import DeviceGraph
    kw.setdefault("solver", "dense")
    return DeviceGraph(robust=None if robust is None or robust[0] is None else robust, **kw)


def _loaded(robust, init, edges, odom=None, **kw):
    dev = _dev(robust, **kw)
    dev.set_poses(init)
    dev.set_edges(edges, odometry=odom)
    return dev


def _base():
    init, truth, rec, cor, _ = rr.corrupted_graph(5)
    assert len(rec) == 264
    return init, truth, rec, cor, gr.odometry(5)


# ------------------------------------------------------------ 1. bit for bit
def test_zero_odometry_edges_is_set_edges():
    """slam_graph_set_edges_odom(h, n, e, 0, NULL) against slam_graph_set_edges:
    one update, then the BSR slots, vals, b, poses and stats, bit for bit."""
    from slamhip import _lib
    init, _, rec, _, _ = _base()
    rec = np.ascontiguousarray(rec)
    old = _loaded(None, init, rec)
    new = _dev()
    try:
        new.set_poses(init)
        _lib.check(new._lib.slam_graph_set_edges_odom(new._h, len(rec), rec.ctypes.data_as(C.c_void_p),
                                                      0, None), "slam_graph_set_edges_odom")
        new.n_edges = len(rec)
        sa, sb = old.update(), new.update()
        assert sa == sb
        for u, v in zip(old.get_bsr(), new.get_bsr()):
            np.testing.assert_array_equal(u, v)
        for u, v in zip(old.get_system(dense=True, blocks=True), new.get_system(dense=True, blocks=True)):
            np.testing.assert_array_equal(u, v)
        np.testing.assert_array_equal(old.get_poses(), new.get_poses())
        np.testing.assert_array_equal(old.get_delta(), new.get_delta())
        for key, val in old.chi2().items():
            assert new.chi2()[key] == val, key
    finally:
        old.close()
        new.close()


@pytest.mark.parametrize("kind,k", [(None, None), ("cauchy", 2.0)], ids=["none", "cauchy2"])
def test_landmark_columns_keep_their_bits(kind, k):
    """The first E_lm columns of a mixed handle's blocks are the blocks of a
    landmark-only handle at the same poses."""
    init, _, _, cor, od = _base()
    mixed = _loaded((kind, k), init, cor, od)
    plain = _loaded((kind, k), init, cor)
    try:
        assert (mixed.n_edges, mixed.n_odom, plain.n_edges, plain.n_odom) == (335, 71, 264, 0)
        mixed.update()
        plain.update()
        blk = mixed.get_system(dense=False, blocks=True)[3]
        blk0 = plain.get_system(dense=False, blocks=True)[3]
        assert blk.shape == (335, 42)
        np.testing.assert_array_equal(blk[:264], blk0)
        if kind is not None:
            for u, v in zip(mixed.edge_weights(), plain.edge_weights()):
                assert u.shape == (335,)
                np.testing.assert_array_equal(u[:264], v)
        # and the odometry edges are in the system
        assert not np.array_equal(mixed.get_poses(), plain.get_poses())
    finally:
        mixed.close()
        plain.close()


def test_device_structure_build_matches_host_on_the_mixed_set():
    init, _, _, cor, od = _base()
    out = []
    for host in (False, True):
        if host:
            os.environ["SLAM_GRAPH_HOST_BUILD"] = "1"
        try:
            dev = _loaded(None, init, cor, od)
            st = dev.update()
            rows, cols, vals = dev.get_bsr()
            times, _, b, _ = dev.get_system(dense=False)
            out.append((rows, cols, vals, times, b, dev.get_poses(), st))
            dev.close()
        finally:
            os.environ.pop("SLAM_GRAPH_HOST_BUILD", None)
    for k, (u, v) in enumerate(zip(*out)):
        if k < 6:
            np.testing.assert_array_equal(u, v)
    assert out[0][6] == out[1][6]


def test_two_handles_and_two_chi2_calls_are_bit_identical():
    init, _, _, cor, od = _base()
    a = _loaded(("cauchy", 2.0), init, cor, od)
    b = _loaded(("cauchy", 2.0), init, cor, od)
    try:
        c1, c2 = a.chi2(per_edge=True), a.chi2(per_edge=True)
        for key in ("chi2", "cost", "max_chi2", "n_low_weight"):
            assert c1[key] == c2[key], key
        np.testing.assert_array_equal(c1["edge_chi2"], c2["edge_chi2"])
        np.testing.assert_array_equal(c1["edge_weight"], c2["edge_weight"])
        sa, sb = a.optimize(0.01, 50), b.optimize(0.01, 50)
        np.testing.assert_array_equal(sa, sb)
        np.testing.assert_array_equal(a.get_poses(), b.get_poses())
    finally:
        a.close()
        b.close()


# ------------------------------------- 2. one update against the restatement
def _one_update(kind, k, n_lm, n_od):
    init, _, _, cor, od = _base()
    rec, odr = cor[:n_lm], od[:n_od]
    edges, orow = rr.edge_rows(rec).reshape(n_lm, 11), gr.odom_rows(odr)
    ref_st, ref_poses, Hr, br, times_r, chi2_r, w_r, delta_r = gr.update_est_pose(edges, orow, init, kind, k)
    blk_r = gr.linearize_odom(orow, init)
    dev = _loaded((kind, k), init, rec, odr)
    try:
        assert (dev.n_edges, dev.n_odom) == (n_lm + n_od, n_od)
        tot = dev.chi2(per_edge=True)
        c, w = tot["edge_chi2"], tot["edge_weight"]
        assert c.shape == (n_lm + n_od,)
        rel = np.abs(c - chi2_r) / np.maximum(chi2_r, 1e-300)
        print(f"chi2: max rel error {rel.max():.3g} (odometry columns {rel[n_lm:].max():.3g})")
        np.testing.assert_allclose(c, chi2_r, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(w, w_r, rtol=2e-9, atol=0)
        assert np.all(w[n_lm:] == 1.0)                       # never down-weighted
        rho = np.concatenate([rr.weight_cost(c[:n_lm], kind, k)[1], c[n_lm:]])
        np.testing.assert_allclose([tot["chi2"], tot["cost"]], [np.sum(c), np.sum(rho)], rtol=1e-12)
        assert tot["max_chi2"] == c.max() and tot["n_low_weight"] == int((w < 0.1).sum())
        st = dev.update()
        times, H, b, blk = dev.get_system(dense=True, blocks=True)
        np.testing.assert_array_equal(times, times_r)
        # the odometry columns of blocks
        tail = blk[n_lm:]
        gap_h = np.abs(tail[:, :36] - blk_r[:, :36]).max() / np.abs(blk_r[:, :36]).max()
        gap_b = np.abs(tail[:, 36:] - blk_r[:, 36:]).max() / np.abs(blk_r[:, 36:]).max()
        print(f"odometry columns: H parts {gap_h:.3g}, b parts {gap_b:.3g} of the column maximum")
        np.testing.assert_allclose(tail[:, :36], blk_r[:, :36], rtol=0, atol=1e-12 * np.abs(blk_r[:, :36]).max())
        np.testing.assert_allclose(tail[:, 36:], blk_r[:, 36:], rtol=0, atol=1e-11 * np.abs(blk_r[:, 36:]).max())
        print(f"H: max error {np.abs(H - Hr).max():.3g} (max |H| {np.abs(Hr).max():.3g}); "
              f"b: max error {np.abs(b - br).max():.3g} (max |b| {np.abs(br).max():.3g})")
        np.testing.assert_allclose(H, Hr, rtol=0, atol=1e-12 * np.abs(Hr).max())
        np.testing.assert_allclose(b, br, rtol=0, atol=1e-11 * np.abs(br).max())
        if kind is not None:
            lc, lw = dev.edge_weights()
            np.testing.assert_array_equal(lc, c)
            np.testing.assert_array_equal(lw, w)
            assert np.all(lw[n_lm:] == 1.0)
        # every case here is solved: the restatement's gate passes with cond(H) <= 2.6e7
        # (the truncated sets included), so no case skips the comparison of delta
        assert ref_st[0] == 1.0 and ref_st[3] < 1e8, (n_lm, n_od, ref_st)
        assert st[0]
        delta = dev.get_delta()
        gap = np.abs(delta - delta_r).max()
        print(f"delta: max error {gap:.3g} (max |delta| {np.abs(delta_r).max():.3g}, cond {ref_st[3]:.3g})")
        assert gap <= ref_st[3] * 1e-12 * np.abs(delta_r).max()
    finally:
        dev.close()


@pytest.mark.parametrize("n_od", E_OD)
@pytest.mark.parametrize("n_lm", E_LM)
@pytest.mark.parametrize("kind,k", [(None, None), ("cauchy", 2.0)], ids=["none", "cauchy2"])
def test_one_update_matches_restatement(kind, k, n_lm, n_od):
    _one_update(kind, k, n_lm, n_od)


@pytest.mark.parametrize("kind,k", [("huber", 1.0), ("dcs", 5.0)], ids=["huber1", "dcs5"])
def test_one_update_matches_restatement_other_kinds(kind, k):
    _one_update(kind, k, 264, 71)


# ------------------------------------------------ 3. Gauss-Newton to the end
@pytest.mark.parametrize("corrupted", [False, True], ids=["clean", "corrupted"])
@pytest.mark.parametrize("seed", [5, 6])
def test_gauss_newton_matches_restatement(seed, corrupted):
    init, truth, rec, cor, _ = rr.corrupted_graph(seed)
    for kind, k in ((None, None), ("cauchy", 2.0)):
        ref_p, ref_st = gr.cpu_run(seed, kind, k, corrupted, True)
        dev = _loaded((kind, k), init, cor if corrupted else rec, gr.odometry(seed))
        try:
            st = dev.optimize(0.01, 50)
            p = dev.get_poses()
        finally:
            dev.close()
        print(f"seed {seed} {'corrupted' if corrupted else 'clean'} {_name(kind, k)}: "
              f"{rr.position_rms(p, truth):.3f} m to truth, {len(st)} iterations, gap to the "
              f"restatement {np.abs(p - ref_p).max():.3g}")
        assert len(st) == len(ref_st) and np.all(st[:, 0] == 1.0)
        np.testing.assert_allclose(p, ref_p, rtol=0, atol=1e-8)


# ------------------------------------------------- 4. the odometry-only chain
def test_odometry_only_chain_closed_form():
    """n_edges = 0, T = 40: the chain has a zero-residual solution; the loop
    reaches it, consecutive poses reproduce rel and the whole trajectory is the
    composition of the rels from pose 0 -- no restatement involved."""
    from slamhip.graph import relpose
    T = 40
    rs = np.random.RandomState(11)
    rel = np.column_stack([rs.uniform(0.5, 1.5, T - 1), rs.uniform(-0.2, 0.2, T - 1),
                           rs.uniform(-0.3, 0.3, T - 1)])
    odom = np.array([[k, k, k + 1, k + 1, *rel[k], 0.02, 0.02, 0.01] for k in range(T - 1)])
    init = np.column_stack([np.cumsum(rs.normal(1.0, 0.3, T)), rs.normal(0, 0.5, T),
                            rs.uniform(-0.5, 0.5, T)])
    from slamhip.graph import EDGE_DTYPE
    dev = _loaded(None, init, np.zeros(0, dtype=EDGE_DTYPE), odom)
    try:
        assert (dev.n_edges, dev.n_odom) == (T - 1, T - 1)
        st = dev.optimize(1e-24, 50)
        poses = dev.get_poses()
        tot = dev.chi2(per_edge=True)
    finally:
        dev.close()
    print(f"chain: {len(st)} iterations, sum chi2 {tot['chi2']:.3g}")
    assert np.all(st[:, 0] == 1.0) and len(st) < 50
    assert tot["chi2"] <= 1e-20 and np.all(tot["edge_weight"] == 1.0)
    closed = np.empty((T, 3))
    closed[0] = poses[0]
    for k in range(T - 1):
        np.testing.assert_allclose(relpose(poses[k], poses[k + 1]), rel[k], rtol=0, atol=1e-12)
        c, s = np.cos(closed[k, 2]), np.sin(closed[k, 2])
        closed[k + 1] = [closed[k, 0] + c * rel[k, 0] - s * rel[k, 1],
                         closed[k, 1] + s * rel[k, 0] + c * rel[k, 1],
                         gr.wrap_angle(closed[k, 2] + rel[k, 2])]
    np.testing.assert_allclose(poses, closed, rtol=0, atol=1e-10)


# ------------------------------------------------------ 5. unobserved poses
def test_unobserved_poses_are_estimated_with_odometry():
    from graph_marginals_ref import ref_columns, unknowns
    init, _, rec, _, od = _base()
    gap = np.arange(30, 36)
    keep = ~(np.isin(rec["time_bfr"], gap) | np.isin(rec["time_aft"], gap))
    pairs = rec[keep]
    assert 0 < len(pairs) < len(rec)
    without = _loaded(None, init, pairs)
    with_od = _loaded(None, init, pairs, od)
    try:
        without.optimize(0.01, 50)
        times0 = without.get_system(dense=False)[0]
        assert not np.isin(gap, times0).any() and len(times0) == 72 - len(gap)
        np.testing.assert_array_equal(without.get_poses()[gap], init[gap])
        st = with_od.optimize(0.01, 50)
        assert np.all(st[:, 0] == 1.0)
        poses = with_od.get_poses()
        assert np.all(np.any(poses[gap] != init[gap], axis=1))
        ok, cov, _ = with_od.marginals([32], relinearize=True, joint=True, symmetrize=False)
        times, H, _, _ = with_od.get_system(dense=True)
        assert len(times) == 72 and ok and np.all(np.isfinite(cov))
        # the bar of test_gpu_graph_marginals.py (dense path) on the H the device exported ...
        q = unknowns(times, np.array([32]))
        _, Xref, spread = ref_columns(H, q)
        bar = max(1e-11 * np.abs(np.linalg.inv(H)).max(), 64 * spread)
        err = np.abs(cov - Xref[q, :]).max()
        # ... and the same bar against the block of the restatement's own inv(H) at these poses
        Hr = gr.update_est_pose(rr.edge_rows(pairs), gr.odom_rows(od), poses)[2]
        np.testing.assert_allclose(H, Hr, rtol=0, atol=1e-12 * np.abs(Hr).max())
        err_r = np.abs(cov - np.linalg.inv(Hr)[np.ix_(q, q)]).max()
        print(f"marginal of time 32: error {err:.3g}, against the restatement's inv(H) {err_r:.3g} "
              f"(bar {bar:.3g}); sigma_xy {np.sqrt(cov[0, 0]):.3g} {np.sqrt(cov[1, 1]):.3g} m")
        assert err <= bar and err_r <= bar
        assert cov[0, 0] > 0 and cov[1, 1] > 0 and cov[2, 2] > 0
    finally:
        without.close()
        with_od.close()


# -------------------------------------------------------------- 6. PCG path
def test_pcg_matches_dense_solver_on_the_mixed_set():
    init, _, _, cor, od = _base()
    dense = _loaded(None, init, cor, od, solver="dense")
    pcg = _loaded(None, init, cor, od, solver="pcg", cond="off", pcg_tol=1e-12)
    try:
        a, b = dense.update(), pcg.update()
        assert a[0] and b[0]
        pa, pb = dense.get_poses(), pcg.get_poses()
        step = np.abs(pa - init).max()
        np.testing.assert_allclose(pb, pa, rtol=0, atol=1e-6 * step)
        np.testing.assert_allclose(b[1], a[1], rtol=1e-6)
        assert pcg.timing()["pcg_iterations"] > 0
        for u, v in zip(dense.get_system(dense=False, blocks=True)[2:], pcg.get_system(dense=False, blocks=True)[2:]):
            np.testing.assert_array_equal(u, v)
    finally:
        dense.close()
        pcg.close()


# ------------------------------------------- 7. argument checks, real handle
def test_record_checks_leave_the_handle():
    """The checks of the records' contents (they need a handle with poses): each
    is SLAM_ERR_ARG naming the entry, and the handle still holds its edge set."""
    from slamhip import _lib
    init, _, _, cor, od = _base()
    dev = _loaded(None, init, cor, od)
    lib = dev._lib
    try:
        before = dev.chi2(per_edge=True)
        rec = np.ascontiguousarray(cor[:10])
        good = np.array(od[:5])

        def call(edges, odom):
            return lib.slam_graph_set_edges_odom(dev._h, len(edges), edges.ctypes.data_as(C.c_void_p),
                                                 len(odom), odom.ctypes.data_as(C.c_void_p))

        def broken(field, value, idx=None):
            bad = good.copy()
            if idx is None:
                bad[field][3] = value
            else:
                bad[field][3, idx] = value
            return bad

        cases = [(rec, broken("pose_aft", 72)), (rec, broken("time_bfr", -1)),
                 (rec, broken("time_aft", good["time_bfr"][3])),
                 (rec, broken("rel", np.nan, 1)), (rec, broken("rel", np.inf, 2)),
                 (rec, broken("sigma", 0.0, 0)), (rec, broken("sigma", -0.1, 1)),
                 (rec, broken("sigma", np.inf, 2)), (rec, broken("sigma", np.nan, 0))]
        bad_rec = rec.copy()
        bad_rec["pose_bfr"][7] = 72
        cases.append((bad_rec, good))
        for edges, odom in cases:
            assert call(edges, odom) == _lib.SLAM_ERR_ARG
            assert "slam_graph_set_edges_odom" in lib.slam_last_error().decode()
        after = dev.chi2(per_edge=True)
        for key in ("chi2", "cost", "max_chi2", "n_low_weight"):
            assert before[key] == after[key], key
        np.testing.assert_array_equal(before["edge_chi2"], after["edge_chi2"])
        assert dev.update()[0]
        assert call(rec, good) == _lib.SLAM_OK
    finally:
        dev.close()


# ------------------------------------------------------------- 8. front end
def _robot_run(odometry, robust=None, steps=12):
    import graph_based_slam as gs
    np.random.seed(7)
    x0 = np.array([[10.0], [0.0], [np.deg2rad(90.0)]])
    rbt = gs.Robot(x0, gs.PERIOD_ms / 1000, gs.SCN_SENS_RANGE_m, gs.SCN_SENS_ANGLE_rps, gs.LAND_MARKS,
                   robust=robust)
    if odometry != "never":
        rbt.setOdometry(odometry)
    for _ in range(steps):
        rbt.move(gs.VEL_mps, gs.OMEGA_rps)
    st = rbt.estimateOpticalTrajectory()
    est = np.array([p[:, 0] for p in rbt._est._poses])
    return rbt, st, est, np.random.rand()


def test_robot_without_odometry_is_unchanged():
    """setOdometry never called against setOdometry(None): the same poses, stats
    and random stream, bit for bit (test_robot_demo_matches_reference holds the
    default path to the reference's golden poses)."""
    _, st_a, est_a, next_a = _robot_run("never")
    _, st_b, est_b, next_b = _robot_run(None)
    np.testing.assert_array_equal(st_a, st_b)
    np.testing.assert_array_equal(est_a, est_b)
    assert next_a == next_b
    # switching odometry on draws nothing either
    assert _robot_run((0.02, 0.02, 0.01))[3] == next_a


def test_robot_with_odometry_covers_every_time():
    rbt, st, est, _ = _robot_run((0.02, 0.02, 0.01), robust=("cauchy", 2.0))
    _, _, est0, _ = _robot_run("never", robust=("cauchy", 2.0))
    dev = rbt._est._dev
    assert dev.n_odom == 12 and dev.n_edges == len(rbt._est._pairs) + 12
    times = dev.get_system(dense=False)[0]
    np.testing.assert_array_equal(times, np.arange(13))
    assert bool(st[-1][0]) and not np.array_equal(est, est0)
    pairs, chi2, w = rbt._est.getEdgeWeights()
    assert len(chi2) == len(w) == len(pairs) > 0
    cov = rbt.getEstTrajCov()
    assert sorted(cov) == list(range(13)) and all(np.all(np.isfinite(c)) for c in cov.values())


def _estimator_with_steps(n_poses, sigma):
    """A TrajectoryEstimator over the first poses of the seed-5 graph, the step
    that led to each pose recorded as its (noisy) odometry."""
    from graph_based_slam import TrajectoryEstimator
    init, _, _, _, od = _base()
    poses = [p.reshape(3, 1).copy() for p in init[:n_poses]]
    te = TrajectoryEstimator(poses[0], solver="dense")
    te.setOdometry(sigma)
    for k in range(1, n_poses):
        te.addPose(poses[k], False, od["rel"][k - 1])
    return te, poses, init[:n_poses], od[:n_poses - 1]


@pytest.mark.parametrize("with_pairs", [True, False], ids=["pairs", "no-pairs"])
def test_update_est_pose_with_odometry(with_pairs):
    """TrajectoryEstimator.updateEstPose with setOdometry, once with pending
    pairs and once with none (odometry only): one update against the
    restatement, and every time of the set written back."""
    from graph_based_slam import HalfEdge, Observation
    T = 20
    te, poses, init, od = _estimator_with_steps(T, gr.SIGMA)
    cor = rr.corrupted_graph(5)[3]
    pairs = cor[(cor["time_aft"] < 12)][:15] if with_pairs else cor[:0]
    for e, r in enumerate(pairs):
        te.setPairObs(HalfEdge(int(r["time_bfr"]), Observation(e, *r["obs_bfr"]), int(r["pose_bfr"])),
                      HalfEdge(int(r["time_aft"]), Observation(e, *r["obs_aft"]), int(r["pose_aft"])))
    assert len(pairs) == (15 if with_pairs else 0)
    ref_st, ref_poses = gr.update_est_pose(rr.edge_rows(pairs).reshape(len(pairs), 11), gr.odom_rows(od),
                                           init)[:2]
    is_calc, dsum, det, cond = te.updateEstPose()
    assert is_calc and ref_st[0] == 1.0
    assert (te._dev.n_edges, te._dev.n_odom) == (len(pairs) + T - 1, T - 1)
    np.testing.assert_array_equal(te._dev.get_system(dense=False)[0], np.arange(T))
    np.testing.assert_allclose(dsum, ref_st[1], rtol=1e-6)
    got = np.hstack(poses).T
    # every time is written back: the caller's arrays hold the device's poses, all
    # of them moved (times 12 .. 19 carry no pair in either case)
    np.testing.assert_array_equal(got, te._dev.get_poses())
    assert np.all(np.any(got[1:] != init[1:], axis=1))
    np.testing.assert_allclose(got, ref_poses, rtol=0, atol=1e-8)
    # the pending pairs are consumed; a second call has the odometry edges alone
    assert te._rows == []
    assert te.updateEstPose()[0] and te._dev.n_edges == T - 1


def test_update_est_pose_without_odometry_and_without_pairs_solves_nothing():
    te, poses, init, _ = _estimator_with_steps(6, None)
    assert te.updateEstPose() == (False, 0.0, 0.0, 0.0)
    np.testing.assert_array_equal(np.hstack(poses).T, init)
