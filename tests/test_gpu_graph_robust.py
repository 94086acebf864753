"""Robust edge weights and the chi-square of the edges on the GPU,
against the NumPy restatement tests/graph_robust_ref.py.

The graphs are the issue's: circle_graph(72, n_landmarks=16, seed) for seeds 5
and 6, one edge in ten given the obs_aft of another edge (a wrong pairing).

Tolerances.  H and b: those of test_gpu_graph.py (atol 1e-12 max|H|, 1e-11
max|b|).  chi2_e: rtol 1e-9, atol 1e-12 -- err carries ~1e-15 of absolute
rounding and Omega's entries are <= ~1e3, so the relative error of chi2 is about
2e-15 / |err|: below 1e-9 for |err| > 2e-6 and below 1e-12 absolute under that.
w_e: rtol 2e-9, since |d ln w| <= 2 |d ln chi2| for all three kinds.  The totals
against np.sum of the device's own per-edge arrays: rtol 1e-12, and bit-identical
between two calls.  Final poses of the Gauss-Newton loop against the
restatement's: atol 1e-8, the bar of test_t300_gauss_newton_loop_matches_reference.
"""
import os
import re

import numpy as np
import pytest

import graph_robust_ref as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [(None, None), ("huber", 1.0), ("cauchy", 2.0), ("dcs", 5.0)]
CASES = list(rr.CASES)          # huber 1.0, huber 2.0, cauchy 2.0, dcs 5.0


def _chi2_threads():
    """Edges per workgroup of graph_chi2_kernel: the kernel's own constant."""
    src = open(os.path.join(ROOT, "slam-robot_simu_amd", "csrc", "graph_kernels.inl")).read()
    return int(re.search(r"constexpr int kChi2Threads = (\d+);", src).group(1))


SIZES = sorted({1, 255, 256, 257, _chi2_threads() + 1})


def _dev(robust=None, **kw):
    from slamhip.graph import DeviceGraph
    kw.setdefault("solver", "dense")
    return DeviceGraph(robust=None if robust is None or robust[0] is None else robust, **kw)


def _loaded(robust, init, edges, **kw):
    dev = _dev(robust, **kw)
    dev.set_poses(init)
    dev.set_edges(edges)
    return dev


def _name(kind, k):
    return "none" if kind is None else "%s%g" % (kind, k)


# ------------------------------------------ 1. one update against the restatement
@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("kind,k", KINDS, ids=[_name(*c) for c in KINDS])
def test_one_update_matches_restatement(kind, k, E):
    init, _, _, cor, _ = rr.corrupted_graph(5)
    assert E <= len(cor)
    rec = cor[:E]
    ref_st, ref_poses, Hr, br, times_r, chi2_r, w_r = rr.update_est_pose(rr.edge_rows(rec), init, kind, k)
    dev = _loaded((kind, k), init, rec)
    try:
        before = dev.chi2(per_edge=True)
        again = dev.chi2(per_edge=True)
        c, w = before["edge_chi2"], before["edge_weight"]
        rel = np.abs(c - chi2_r) / np.maximum(chi2_r, 1e-300)
        print(f"chi2: max rel error {rel.max():.3g}; w: max rel error {(np.abs(w - w_r) / w_r).max():.3g}")
        np.testing.assert_allclose(c, chi2_r, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(w, w_r, rtol=2e-9, atol=0)
        # the totals: the device's own arrays, summed; bit-identical call to call
        rho = rr.weight_cost(c, kind, k)[1]
        np.testing.assert_allclose([before["chi2"], before["cost"]], [np.sum(c), np.sum(rho)], rtol=1e-12)
        assert before["max_chi2"] == c.max() and before["n_low_weight"] == int((w < 0.1).sum())
        for key in ("chi2", "cost", "max_chi2", "n_low_weight"):
            assert before[key] == again[key], key
        np.testing.assert_array_equal(again["edge_chi2"], c)
        np.testing.assert_array_equal(again["edge_weight"], w)
        # the update: weighted blocks, assembled
        st = dev.update()
        times, H, b, blk = dev.get_system(dense=True, blocks=True)
        np.testing.assert_array_equal(times, times_r)
        print(f"H: max error {np.abs(H - Hr).max():.3g} (max |H| {np.abs(Hr).max():.3g}); "
              f"b: max error {np.abs(b - br).max():.3g} (max |b| {np.abs(br).max():.3g})")
        np.testing.assert_allclose(H, Hr, rtol=0, atol=1e-12 * np.abs(Hr).max())
        np.testing.assert_allclose(b, br, rtol=0, atol=1e-11 * np.abs(br).max())
        if kind is not None:
            lc, lw = dev.edge_weights()
            np.testing.assert_array_equal(lc, c)
            np.testing.assert_array_equal(lw, w)
        if ref_st[3] < 1e12:
            assert st[0] == bool(ref_st[0])
    finally:
        dev.close()


# --------------------------------------------------------------- 2. chi2 = 0
def test_zero_residual_edge_has_unit_weight_and_the_plain_blocks():
    """An edge between two equal poses with equal observations: err = 0 exactly,
    so chi2 = 0, w = 1 (not 0 / 0) and its 42 values are those of the plain kernel."""
    from slamhip.graph import EDGE_DTYPE
    init, _, _, cor, _ = rr.corrupted_graph(5)
    poses = np.array(init)
    poses[71] = poses[3]
    zero = np.zeros(1, dtype=EDGE_DTYPE)
    zero["time_bfr"], zero["pose_bfr"], zero["time_aft"], zero["pose_aft"] = 3, 3, 71, 71
    zero["obs_bfr"] = zero["obs_aft"] = [6.5, 0.3, -1.1]
    rec = np.concatenate([cor[:20], zero])
    plain = _loaded(None, poses, rec)
    try:
        tot0 = plain.chi2(per_edge=True)        # before the update moves the two poses apart
        plain.update()
        blk0 = plain.get_system(dense=False, blocks=True)[3]
        assert tot0["edge_chi2"][-1] == 0.0 and tot0["edge_weight"][-1] == 1.0
        assert np.all(tot0["edge_weight"] == 1.0) and tot0["chi2"] == tot0["cost"]
    finally:
        plain.close()
    for kind, k in CASES:
        dev = _loaded((kind, k), poses, rec)
        try:
            dev.update()
            blk = dev.get_system(dense=False, blocks=True)[3]
            c, w = dev.edge_weights()
            assert c[-1] == 0.0 and w[-1] == 1.0, (kind, k)
            # every edge of weight 1 keeps the plain kernel's bits, the others do not
            np.testing.assert_array_equal(blk[w == 1.0], blk0[w == 1.0])
            assert np.all(np.any(blk[w < 1.0] != blk0[w < 1.0], axis=1))
            if kind == "cauchy":
                assert np.all(w[:-1] < 1.0)
        finally:
            dev.close()


# ---------------------------------------------------- 3. the default is untouched
def test_default_path_is_bit_identical():
    init, _, _, cor, _ = rr.corrupted_graph(5)
    never = _loaded(None, init, cor)
    none = _loaded(None, init, cor)
    back = _loaded(None, init, cor)
    try:
        none.set_robust("none")
        back.set_robust("cauchy", 2.0)
        back.update()                           # a weighted step in between
        back.set_robust(None)
        back.set_poses(init)
        systems = []
        for d in (never, none, back):
            d.update()
            systems.append(d.get_system(dense=True, blocks=True))
        for s in systems[1:]:
            for u, v in zip(systems[0], s):
                np.testing.assert_array_equal(u, v)
        finals = []
        for d in (never, none, back):
            d.set_poses(init)
            st = d.optimize(0.01, 50)
            finals.append((st, d.get_poses()))
        for st, p in finals[1:]:
            np.testing.assert_array_equal(st, finals[0][0])
            np.testing.assert_array_equal(p, finals[0][1])
        # and a cauchy handle is not the default
        back.set_robust("cauchy", 2.0)
        back.set_poses(init)
        back.update()
        assert not np.array_equal(back.get_system(dense=True)[1], systems[0][1])
    finally:
        for d in (never, none, back):
            d.close()


# --------------------------------------------- 4. the stored rows, and what chi2 leaves
def test_edge_weights_are_those_of_the_last_linearisation():
    from slamhip import _lib
    init, _, _, cor, _ = rr.corrupted_graph(5)
    dev = _loaded(("cauchy", 2.0), init, cor)
    try:
        with pytest.raises(RuntimeError, match="nothing linearised"):
            dev.edge_weights()
        for _ in range(2):
            p0 = dev.get_poses()
            before = dev.chi2(per_edge=True)
            assert dev.update()[0]
            c, w = dev.edge_weights()
            np.testing.assert_array_equal(c, before["edge_chi2"])
            np.testing.assert_array_equal(w, before["edge_weight"])
            # chi2 moves nothing: poses, delta, system, timing, and the stored rows
            state = (dev.get_poses(), dev.get_delta(), dev.get_system(dense=True, blocks=True),
                     dev.timing())
            after = dev.chi2(per_edge=True)
            assert not np.array_equal(after["edge_chi2"], c) and not np.array_equal(state[0], p0)
            np.testing.assert_array_equal(dev.get_poses(), state[0])
            np.testing.assert_array_equal(dev.get_delta(), state[1])
            for u, v in zip(dev.get_system(dense=True, blocks=True), state[2]):
                np.testing.assert_array_equal(u, v)
            assert dev.timing() == state[3]
            c2, w2 = dev.edge_weights()
            np.testing.assert_array_equal(c2, c)
            np.testing.assert_array_equal(w2, w)
        # a new edge set forgets the rows; the argument checks on a real handle
        dev.set_edges(cor[:10])
        with pytest.raises(RuntimeError, match="nothing linearised"):
            dev.edge_weights()
        lib = _lib.load()
        for kind, param in ((4, 1.0), (1, float("nan")), (1, 0.0), (3, -2.0)):
            assert lib.slam_graph_set_robust(dev._h, kind, param) == _lib.SLAM_ERR_ARG
        assert lib.slam_graph_chi2(dev._h, None, None, None) == _lib.SLAM_ERR_ARG
        # the rejected calls left the kind: still cauchy 2.0
        assert dev.chi2(per_edge=True)["edge_weight"].min() < 1.0
        # kind none stores no rows: a clear error
        dev.set_robust(None)
        dev.update()
        with pytest.raises(RuntimeError, match="kind none"):
            dev.edge_weights()
        # no edges: SLAM_OK with the totals zero
        dev.set_edges(cor[:0])
        assert dev.chi2() == dict(chi2=0.0, cost=0.0, max_chi2=0.0, n_low_weight=0)
    finally:
        dev.close()


# ------------------------------------------------------------ 5. end to end
_device_runs = {}


def _device_run(seed, kind, k, corrupted=True):
    """Gauss-Newton on the device (dense path), once per case: final poses, the
    per-iteration stats, chi2 and w at the final poses."""
    key = (seed, kind, k, corrupted)
    if key not in _device_runs:
        init, _, rec, cor, _ = rr.corrupted_graph(seed)
        dev = _loaded((kind, k), init, cor if corrupted else rec)
        try:
            st = dev.optimize(0.01, 50)
            fin = dev.chi2(per_edge=True)
            _device_runs[key] = (dev.get_poses(), st, fin["edge_chi2"], fin["edge_weight"])
        finally:
            dev.close()
    return _device_runs[key]


@pytest.mark.parametrize("seed", [5, 6])
def test_end_to_end_dense(seed):
    mask = rr.corrupted_graph(seed)[4]
    clean, st0, _, _ = _device_run(seed, None, None, corrupted=False)
    plain, st1, _, _ = _device_run(seed, None, None)
    assert np.all(st0[:, 0] == 1.0) and np.all(st1[:, 0] == 1.0)
    d_plain = rr.position_rms(plain, clean)
    for kind, k in CASES:
        p, st, chi2, w = _device_run(seed, kind, k)
        assert np.all(st[:, 0] == 1.0) and len(st) < 50
        d = rr.position_rms(p, clean)
        ref = rr.cpu_run(seed, kind, k)[0]
        gap = np.abs(p - ref).max()
        low = w < 0.1
        print(f"seed {seed} {kind} {k}: to clean {d:.4f} m (plain {d_plain:.4f} m, ratio "
              f"{d_plain / d:.2f}), {len(st)} iterations, w < 0.1: {int((low & mask).sum())} of "
              f"{int(mask.sum())} corrupted, {int((low & ~mask).sum())} clean; gap to the "
              f"restatement {gap:.3g}")
        assert d <= d_plain / 3.0, (seed, kind, k, d, d_plain)
        if seed == 5 and (kind, k) in (("cauchy", 2.0), ("dcs", 5.0)):
            assert mask.sum() == 26
            assert (low & mask).sum() >= 24 and (low & ~mask).sum() <= 8, (kind, k)
        np.testing.assert_allclose(p, ref, rtol=0, atol=1e-8)


# -------------------------------------------------------------- 6. PCG path
def test_pcg_matches_dense_solver_with_weights():
    init, _, _, cor, _ = rr.corrupted_graph(5)
    dense = _loaded(("cauchy", 2.0), init, cor, solver="dense")
    pcg = _loaded(("cauchy", 2.0), init, cor, solver="pcg", pcg_tol=1e-12)
    try:
        a = dense.update()
        b = pcg.update()
        assert a[0] and b[0]
        pa, pb = dense.get_poses(), pcg.get_poses()
        step = np.abs(pa - init).max()
        np.testing.assert_allclose(pb, pa, rtol=0, atol=1e-6 * step)
        np.testing.assert_allclose(b[1], a[1], rtol=1e-6)
        assert (b[2] > 0.1) == (a[2] > 0.1) and abs(b[3] / a[3] - 1) < 3e-2, (a, b)
        assert pcg.timing()["pcg_iterations"] > 0
        for u, v in zip(dense.edge_weights(), pcg.edge_weights()):
            np.testing.assert_array_equal(u, v)
    finally:
        dense.close()
        pcg.close()


# ------------------------------------------------------------- 7. marginals
def test_marginals_are_blocks_of_the_weighted_inverse():
    from graph_marginals_ref import ref_columns, unknowns
    init, _, _, cor, _ = rr.corrupted_graph(5)
    dev = _loaded(("cauchy", 2.0), init, cor)
    plain = _loaded(None, init, cor)
    try:
        dev.optimize(0.01, 50)
        plain.set_poses(dev.get_poses())
        times = np.array([0, 17, 40, 71])
        ok, cov, _ = dev.marginals(times, relinearize=True, joint=True, symmetrize=False)
        assert ok
        all_times, H, _, _ = dev.get_system(dense=True)
        q = unknowns(all_times, times)
        _, Xref, spread = ref_columns(H, q)
        bar = max(1e-11 * np.abs(np.linalg.inv(H)).max(), 64 * spread)
        err = np.abs(cov - Xref[q, :]).max()
        print(f"weighted marginals: max error {err:.3g}, bar {bar:.3g}")
        assert err <= bar
        # the weighted H at these poses, not the plain one
        c, w = dev.edge_weights()
        np.testing.assert_array_equal(w, dev.chi2(per_edge=True)["edge_weight"])
        ok0, cov0, _ = plain.marginals(times, relinearize=True, joint=True, symmetrize=False)
        assert ok0 and np.abs(cov - cov0).max() > 100 * bar
    finally:
        dev.close()
        plain.close()


# --------------------------------------------------------------- 8. drop-in
def test_trajectory_estimator_names_the_rejected_pairings():
    """Half-edges of the seed-5 graph, one landmark id per edge, so the pairing
    by id rebuilds the edge list -- the corrupted edges are pairs whose id joins
    observations that do not belong together."""
    from graph_based_slam import HalfEdge, Observation, TrajectoryEstimator
    init, _, _, cor, mask = rr.corrupted_graph(5)
    halves = []
    for e, r in enumerate(cor):
        halves.append(HalfEdge(int(r["time_bfr"]), Observation(e, *r["obs_bfr"]), int(r["pose_bfr"])))
        halves.append(HalfEdge(int(r["time_aft"]), Observation(e, *r["obs_aft"]), int(r["pose_aft"])))
    poses = [p.reshape(3, 1).copy() for p in init]
    te = TrajectoryEstimator(poses[0], solver="dense", robust=("cauchy", 2.0))
    assert te.getEdgeWeights() is None
    for p in poses[1:]:
        te.addPose(p, True)
    st = te.estimate_trajectory(halves, len(cor), max_iter=50)
    pairs, chi2, w = te.getEdgeWeights()
    assert len(pairs) == len(cor)
    for field in cor.dtype.names:                           # the order of the pair list
        np.testing.assert_array_equal(pairs[field], cor[field])
    ref_p, ref_st, _, _ = _device_run(5, "cauchy", 2.0)
    np.testing.assert_array_equal(st, ref_st)
    np.testing.assert_array_equal(np.hstack(poses).T, ref_p)
    # the rows of the loop's last linearisation: one more step would use them
    dev = _loaded(("cauchy", 2.0), init, cor)
    try:
        dev.optimize(0.01, 50)
        for u, v in zip(dev.edge_weights(), (chi2, w)):
            np.testing.assert_array_equal(u, v)
    finally:
        dev.close()
    low = w < 0.1
    assert (low & mask).sum() >= 24 and (low & ~mask).sum() <= 8
