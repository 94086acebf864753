"""Marginal covariances of selected poses (slam_graph_marginals) on the GPU.

The reference is tests/graph_marginals_ref.py: columns of NumPy's inverse,
refined with extended-precision residuals, on the H the device exported (or
the reference's own H for the golden demo iterations); ``spread`` is that
reference's own error.  Two bars:

* dense path: |error| <= max(1e-11 max|Sigma|, 64 spread) -- the lockstep
  convention of the dense solver's tests (an LU in float64 on the same H);
* PCG path: |error| <= pcg_tol / lambda_min(sym H) + 64 spread, with pcg_tol =
  1e-12: ||x - x*|| <= ||r|| / lambda_min for a unit right-hand side, plus the
  drift of the recurrence residual.
"""
import ctypes as C
import os

import numpy as np
import pytest

import graph_oracle as go
from conftest import golden
from graph_marginals_ref import ref_columns, unknowns

pytestmark = pytest.mark.gpu

PCG_TOL = 1e-12
DEFAULT_COLS = 4           # columns per pass of the PCG path
ANCHOR = 1e4


def _dev(**kw):
    from slamhip.graph import DeviceGraph
    if kw.get("solver") == "pcg":
        kw.setdefault("pcg_tol", PCG_TOL)
    return DeviceGraph(**kw)


def _bar(H, spread, solver):
    if solver == "dense":
        return max(1e-11 * np.abs(np.linalg.inv(H)).max(), 64 * spread)
    lam_min = np.linalg.eigvalsh(0.5 * (H + H.T))[0]
    assert lam_min > 0
    return PCG_TOL / lam_min + 64 * spread


def _check(cov, H, all_times, times, solver, what):
    """cov (3m, 3m) against the refined columns of inv(H); returns the bar."""
    q = unknowns(all_times, times)
    _, Xref, spread = ref_columns(H, q)
    bar = _bar(H, spread, solver)
    err = np.abs(cov - Xref[q, :]).max()
    print(f"{what}: max error {err:.3g}, bar {bar:.3g}, spread {spread:.3g}")
    assert err <= bar, (what, err, bar)
    return bar


_graphs = {}


def _circle(n):
    from slamhip.graph import circle_graph
    if n not in _graphs:
        _graphs[n] = circle_graph(n, n_landmarks=24, seed=n)
    return _graphs[n]


def _circle_dev(n, solver, **kw):
    init, _, edges = _circle(n)
    dev = _dev(solver=solver, **kw)
    dev.set_poses(init)
    dev.set_edges(edges)
    return dev


def _state(dev):
    return dev.get_poses(), dev.get_delta(), dev.timing(), dev.cond_info(), dev.gate_info()


def _same_state(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2] and a[3] == b[3]
    assert repr(a[4]) == repr(b[4])              # gate_info holds NaN: compare the text


# ------------------------------------------------ 1. the reference's matrix
@pytest.mark.parametrize("solver", ["dense", "pcg"])
def test_demo_iterations_against_reference_matrix(solver):
    g = golden("graph")
    dev = _dev(solver=solver)
    try:
        for i in sorted({3, 50, int(g["demo_n"]) - 1}):
            dev.set_poses(g[f"demo{i}_poses_before"])
            dev.set_edges(go.edges_from_pairs(g[f"demo{i}_pairs"]))
            dev.update()
            times = g[f"demo{i}_times"]
            ok, cov, info = dev.marginals(times, relinearize=False, joint=True, symmetrize=False)
            assert ok, (i, info)
            assert cov.shape == (3 * len(times), 3 * len(times))
            _check(cov, g[f"demo{i}_H"], times, times, solver, f"demo{i} {solver}")
    finally:
        dev.close()


def test_singular_demo_iteration_is_not_calculable():
    g = golden("graph")
    dev = _dev(solver="dense")
    try:
        dev.set_poses(g["demo20_poses_before"])
        dev.set_edges(go.edges_from_pairs(g["demo20_pairs"]))
        assert dev.update()[0] is False
        ok, cov, info = dev.marginals(g["demo20_times"], relinearize=False, joint=True)
        assert ok is False and np.all(np.isnan(cov))
    finally:
        dev.close()


# ------------------------------------------------ 2. workgroup and pass edges
@pytest.mark.parametrize("m", [1, 4, "R/3+1"])
@pytest.mark.parametrize("n,solver", [(65, "pcg"), (65, "dense"), (129, "pcg"), (300, "pcg"),
                                      (300, "dense")])
def test_workgroup_and_pass_edges(n, solver, m):
    dev = _circle_dev(n, solver)
    try:
        first, second, middle, last = 0, 1, n // 2, n - 1
        if m == "R/3+1":
            default_cols = dev.marginals([first])[2]["cols"] if solver == "pcg" else DEFAULT_COLS
            assert default_cols == DEFAULT_COLS
            m = default_cols // 3 + 1
            times = [last, first, middle][:m]
        else:
            times = [first, second, middle, last][:m]
        ok, cov, info = dev.marginals(times, joint=True, symmetrize=False)
        all_times, H, _, _ = dev.get_system()            # relinearize=True: the system used
        assert len(all_times) == n
        assert ok, info
        if solver == "pcg":
            assert info["cols"] == DEFAULT_COLS and info["passes"] == -(-3 * m // DEFAULT_COLS)
            assert 0 < info["iterations"] and info["residual"] <= PCG_TOL
        bar = _check(cov, H, all_times, times, solver, f"circle {n} {solver} m={m}")
        # The first pose's marginal is (anchor I + S)^-1, S the edges' Schur
        # complement on it.  Every edge Jacobian has identity x, y columns
        # (graph_based_slam.py:404-413), so a common translation is in the null
        # space of the edges' H whatever the residuals are: S = s e_th e_th^T and
        # the block is diag(1 / anchor, 1 / anchor, 1 / (anchor + s)).  A common
        # rotation is in it only at zero residual (J g = the edge's error), so
        # with noisy observations s > 0: the host oracle's own inverse gives
        # 9.74e-5 (n = 65) and 9.69e-5 (n = 300) for the heading entry, not 1e-4.
        a = times.index(first)
        blk = cov[3 * a:3 * a + 3, 3 * a:3 * a + 3]
        want = np.identity(3) / ANCHOR
        off_heading = np.ones((3, 3), dtype=bool)
        off_heading[2, 2] = False
        assert np.abs(blk - want)[off_heading].max() <= bar
        assert 0 < blk[2, 2] <= 1 / ANCHOR + bar
        # the per-pose form and the host symmetrisation
        ok2, cov3, _ = dev.marginals(times)
        assert ok2 and cov3.shape == (m, 3, 3)
        sym = 0.5 * (cov + cov.T)
        for k in range(m):
            np.testing.assert_array_equal(cov3[k], sym[3 * k:3 * k + 3, 3 * k:3 * k + 3])
    finally:
        dev.close()


# ------------------------------------------------ 3. sparse times
def _sparse_times_graph():
    """The sparse_times construction of test_device_structure_build_matches_host:
    a subset of the times, repeated pairs, edges within one time, unsorted."""
    from slamhip.graph import edge_array
    rs = np.random.RandomState(9)
    T = 400
    init = np.column_stack([rs.uniform(-5, 5, T), rs.uniform(-5, 5, T), rs.uniform(-3, 3, T)])
    used = np.sort(rs.choice(T, 120, replace=False))
    rows = []
    for _ in range(900):
        a, c = used[rs.randint(len(used))], used[rs.randint(len(used))]
        if rs.rand() < 0.05:
            c = a
        rows.append([a, a, rs.uniform(1, 9), rs.uniform(-1, 1), rs.uniform(-3, 3),
                     c, c, rs.uniform(1, 9), rs.uniform(-1, 1), rs.uniform(-3, 3)])
    return init, used, edge_array(rows)


@pytest.mark.parametrize("solver", ["pcg", "dense"])
def test_sparse_times_by_value_and_bad_times(solver):
    from slamhip._lib import SLAM_ERR_ARG, SlamError
    init, used, edges = _sparse_times_graph()
    dev = _dev(solver=solver)
    try:
        dev.set_poses(init)
        dev.set_edges(edges)
        dev.update()
        times = [int(used[60]), int(used[0]), int(used[-1]), int(used[7])]
        ok, cov, info = dev.marginals(times, joint=True, symmetrize=False)
        all_times, H, _, _ = dev.get_system()
        np.testing.assert_array_equal(all_times, used)
        assert ok, info
        _check(cov, H, all_times, times, solver, f"sparse times {solver}")
        before = _state(dev)
        absent = int(np.setdiff1d(np.arange(400), used)[3])
        for bad in ([times[0], absent], [times[0], times[1], times[0]], [-1], [400]):
            with pytest.raises(SlamError) as e:
                dev.marginals(bad)
            assert e.value.code == SLAM_ERR_ARG
        _same_state(before, _state(dev))
    finally:
        dev.close()


# ------------------------------------------------ 4. column independence, bitwise
def test_columns_do_not_depend_on_their_company():
    n = 300
    dev = _circle_dev(n, "pcg")
    try:
        a, b, c, d, e = 17, 150, 0, 299, 64
        runs = {}
        for cols in (0, 1, 2, 8):
            dev.set_marginal_cols(cols)
            ok1, two, i1 = dev.marginals([a, b], joint=True, symmetrize=False)
            ok2, five, i2 = dev.marginals([b, c, a, d, e], joint=True, symmetrize=False)
            ok3, again, _ = dev.marginals([b, c, a, d, e], joint=True, symmetrize=False)
            assert ok1 and ok2 and ok3
            assert i1["cols"] == (cols or DEFAULT_COLS)
            assert i2["passes"] == -(-15 // (cols or DEFAULT_COLS))
            np.testing.assert_array_equal(five, again)
            # [a, b] inside [b, c, a, d, e]: a is entry 2, b entry 0
            pick = np.r_[6:9, 0:3]
            np.testing.assert_array_equal(two, five[np.ix_(pick, pick)])
            runs[cols] = (two, five)
        for cols in (1, 2, 8):
            np.testing.assert_array_equal(runs[0][0], runs[cols][0])
            np.testing.assert_array_equal(runs[0][1], runs[cols][1])
        # the one-workgroup fold launch (the A/B's other form) folds in the same order
        dev.set_marginal_cols(0)
        os.environ["SLAM_GRAPH_MARG_FOLD"] = "1"
        try:
            ok, five, _ = dev.marginals([b, c, a, d, e], joint=True, symmetrize=False)
        finally:
            os.environ.pop("SLAM_GRAPH_MARG_FOLD", None)
        assert ok
        np.testing.assert_array_equal(five, runs[0][1])
    finally:
        dev.close()


# ------------------------------------------------ 5. relinearize and state
# (the dense LU of 900 unknowns takes ~0.5 s a call: the dense case runs at 129 poses)
@pytest.mark.parametrize("solver,n", [("pcg", 300), ("dense", 129)])
def test_relinearize_and_state(solver, n):
    dev, twin = _circle_dev(n, solver), _circle_dev(n, solver)
    try:
        assert dev.update()[0] and twin.update()[0]
        times = [0, n // 2, n - 1]
        all_times, H0, _, _ = dev.get_system()
        before = _state(dev)
        ok0, cov0, _ = dev.marginals(times, relinearize=False, joint=True, symmetrize=False)
        assert ok0
        np.testing.assert_array_equal(dev.get_system()[1], H0)       # the last assembled system
        _same_state(before, _state(dev))
        ok1, cov1, _ = dev.marginals(times, relinearize=True, joint=True, symmetrize=False)
        assert ok1
        H1 = dev.get_system()[1]
        _same_state(before, _state(dev))
        bar0 = _check(cov0, H0, all_times, times, solver, f"relinearize=False {solver}")
        bar1 = _check(cov1, H1, all_times, times, solver, f"relinearize=True {solver}")
        assert np.abs(cov1 - cov0).max() > max(bar0, bar1)           # the poses moved
        # the next update is the one a handle that never asked would make
        st, st_twin = dev.update(), twin.update()
        np.testing.assert_array_equal(st, st_twin)
        np.testing.assert_array_equal(dev.get_poses(), twin.get_poses())
    finally:
        dev.close()
        twin.close()


def test_relinearize_false_needs_an_assembled_system():
    from slamhip._lib import SLAM_ERR_ARG, SlamError
    dev = _circle_dev(65, "pcg")
    try:
        with pytest.raises(SlamError) as e:
            dev.marginals([0], relinearize=False)
        assert e.value.code == SLAM_ERR_ARG
        assert dev.marginals([0], relinearize=True)[0]
        assert dev.marginals([0], relinearize=False)[0]
    finally:
        dev.close()


# ------------------------------------------------ 6. iteration cap
@pytest.mark.parametrize("cap", [1, 17])
def test_iteration_cap_is_not_an_error(cap):
    dev = _circle_dev(300, "pcg", pcg_tol=1e-14, pcg_max_iter=cap)
    try:
        dev.update()                                   # is_calc = 0 at this cap: poses stay
        before = _state(dev)
        ok, cov, info = dev.marginals([0, 150, 299], joint=True)     # SLAM_OK: no exception
        assert ok is False and np.all(np.isnan(cov))
        assert info["iterations"] == cap and info["passes"] == 1
        _same_state(before, _state(dev))
    finally:
        dev.close()


# ------------------------------------------------ 7. front end
def test_trajectory_estimator_covariances():
    from graph_based_slam import HalfEdge, Observation, TrajectoryEstimator
    from slamhip import _lib
    g = golden("graph")
    halves = [HalfEdge(int(h[0]), Observation(int(h[2]), h[3], h[4], h[5]), int(h[1]))
              for h in g["big_halves"]]
    poses = [p.reshape(3, 1).copy() for p in g["big0_poses_before"]]
    te = TrajectoryEstimator(poses[0])
    assert te.getEstTrajCov() is None                  # nothing solved yet
    for p in poses[1:]:
        te.addPose(p, True)
    st = te.estimate_trajectory(halves, 9)
    assert st[-1][0] == 1.0
    solved = te._dev.get_system(dense=False)[0]              # the times of the solved edge set
    assert len(solved) > 10
    covs = te.getEstTrajCov()
    assert sorted(covs) == solved.tolist()
    ok, direct, _ = te._dev.marginals(solved)
    assert ok
    lib = _lib.load()
    for k, t in enumerate(solved):
        S = covs[t]
        assert S.shape == (3, 3)
        np.testing.assert_array_equal(S, S.T)
        assert np.linalg.eigvalsh(S)[0] > 0
        np.testing.assert_array_equal(S, direct[k])
    # the 2x2 position corners through the device ellipse routine
    corners = np.ascontiguousarray(np.stack([covs[t][0:2, 0:2] for t in solved]))
    out = np.zeros((len(solved), 3))
    _lib.check(lib.slam_error_ellipse(len(solved), _lib.dptr(corners), 3.0, 0, _lib.dptr(out), 0),
               "slam_error_ellipse")
    assert np.all(np.isfinite(out)) and np.all(out[:, :2] > 0)
    sub = te.getEstTrajCov([int(solved[-1]), int(solved[0])])
    np.testing.assert_array_equal(sub[int(solved[0])], covs[int(solved[0])])


# ------------------------------------------------ 8. lifetime
def test_marginal_buffers_are_released():
    from slamhip import _lib
    from slamhip.graph import DeviceGraph

    def live():
        out = (C.c_int64 * 3)()
        _lib.check(_lib.load().slam_debug_live_resources(out), "slam_debug_live_resources")
        return tuple(out)

    import gc
    gc.collect()
    first = live()
    for solver in ("pcg", "dense"):
        dev = DeviceGraph(solver=solver, pcg_tol=PCG_TOL)
        init, _, edges = _circle(65)
        dev.set_poses(init)
        dev.set_edges(edges)
        c0 = live()
        assert dev.marginals([0, 64])[0]
        c1 = live()
        assert c1[0] > c0[0] and c1[1] > c0[1] and c1[2] > c0[2]     # allocated on first use
        assert dev.marginals([64, 3])[0]
        assert live() == c1                                          # and reused
        init, _, edges = _circle(300)                                # grow on the same handle
        dev.set_poses(init)
        dev.set_edges(edges)
        c2 = live()
        assert dev.marginals([0, 150, 299, 7])[0]
        c3 = live()
        assert c3[0] > c2[0] and c3[1:] == c2[1:]
        dev.close()
        assert live() == first
