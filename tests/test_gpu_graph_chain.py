"""The chain preconditioner of the graph estimator's PCG on the GPU
against the NumPy restatement tests/graph_chain_ref.py.  Every handle here forces
``solver="pcg"`` unless the test is about the dense path.

The apply: M is built from the handle's own get_bsr values and z = M^-1 r is held
to cond(M) * 1e-12 * max|z| (cond from NumPy), the form the project uses for
delta.  Largest gap / bar found over all cases, segments and both vectors: see
DESIGN 8.5.  Segment 1 against block-Jacobi's apply_precond: both run the same
inv3_lu and the same three-term product in the same order, so they should agree
to the bit; the test allows 4 ulps of the pose's largest |z| and prints what it
finds.

The solve: the systems of DESIGN 8.5's CPU table at T = 72 and T = 300 with
odometry edges, from the initial poses.  delta against the restatement's dense
-H^-1 b: the bar of test_gpu_graph_odom.py's PCG test, 1e-6 of the largest step
at pcg_tol = 1e-12.  Final poses of the Gauss-Newton loop against block-Jacobi's:
atol 1e-8, the bar of the other graph tests.  Iteration counts at the table's
tol 1e-10: chain S = 64 at most a quarter of the device's own block-Jacobi count
(the CPU table's ratios are 7.8 and 8.1).
"""
import numpy as np
import pytest

import graph_chain_ref as cr

pytestmark = pytest.mark.gpu

SEGS = (1, 2, 4, 64)


def _dev(name_or_case, precond=None, **kw):
    from slamhip.graph import DeviceGraph
    poses, rec, od, robust = cr.case(name_or_case) if isinstance(name_or_case, str) else name_or_case
    kw.setdefault("solver", "pcg")
    kw.setdefault("cond", "off")
    dev = DeviceGraph(robust=robust, **kw)
    try:
        if precond != "untouched":
            dev.set_precond(precond)
        dev.set_poses(poses)
        dev.set_edges(rec, odometry=od if len(od) else None)
    except Exception:
        dev.close()
        raise
    return dev


def _table_case(T):
    import graph_odom_ref as gr
    from slamhip.graph import circle_graph, circle_graph_odometry
    init, truth, rec = circle_graph(T, n_landmarks=64, seed=0, odom_noise=0.002)
    return init, rec, circle_graph_odometry(truth, gr.SIGMA, 0), None


def _m_of(dev, S):
    times = dev.get_system(dense=False)[0]
    rows, cols, vals = dev.get_bsr()
    nt = len(times)
    want = int(np.sum((cols == rows + 1) & (rows // S == cols // S)))
    return cr.build_m(rows, cols, vals, nt, S), nt, want


# ------------------------------------------- 1. the apply against the restatement
@pytest.mark.parametrize("name", cr.CASES)
def test_apply_matches_restatement(name):
    dev = _dev(name)
    rs = np.random.RandomState(17)
    worst = 0.0
    try:
        for S in SEGS:
            dev.set_precond("chain", S)
            st = dev.update()                      # linearises: the segment takes effect
            assert st[0], (name, S)
            info = dev.precond_info()
            M, nt, want = _m_of(dev, S)
            assert info == dict(kind="chain", segment=S, off_diagonal_blocks=want, bad_pivots=0)
            if name == "gaps":
                rows, cols, _ = dev.get_bsr()
                slots = set(zip(rows.tolist(), cols.tolist()))
                assert all((a, b) not in slots for a, b in cr.GAPS)
            if name == "even_times":
                np.testing.assert_array_equal(dev.get_system(dense=False)[0], 2 * np.arange(nt))
            b = dev.get_system(dense=False)[2]
            cond = np.linalg.cond(M)
            for r in (-b, rs.standard_normal(3 * nt)):
                z = dev.apply_precond(r)
                ref = np.linalg.solve(M, r)
                bar = cond * 1e-12 * np.abs(ref).max()
                gap = np.abs(z - ref).max()
                worst = max(worst, gap / bar)
                assert gap <= bar, (name, S, gap, bar, cond)
        print(f"{name}: largest gap / bar {worst:.3g}")
    finally:
        dev.close()


@pytest.mark.parametrize("name", ["odom65", "mixed200", "cauchy"])
def test_segment_one_is_block_jacobi(name):
    one = _dev(name, ("chain", 1))
    bj = _dev(name, "block_jacobi")
    try:
        assert one.update()[0] and bj.update()[0]
        np.testing.assert_array_equal(one.get_bsr()[2], bj.get_bsr()[2])
        assert bj.precond_info() == dict(kind="block_jacobi", segment=1, off_diagonal_blocks=0,
                                         bad_pivots=0)
        b = bj.get_system(dense=False)[2]
        # block-Jacobi's apply is minv r
        _, _, vals = bj.get_bsr()
        rows, cols, _ = bj.get_bsr()
        D = vals[rows == cols]
        zb = bj.apply_precond(-b)
        ref = np.einsum("kij,kj->ki", np.linalg.inv(D), (-b).reshape(-1, 3)).reshape(-1)
        np.testing.assert_allclose(zb, ref, rtol=0, atol=np.linalg.cond(D).max() * 1e-12 * np.abs(ref).max())
        for r in (-b, np.random.RandomState(3).standard_normal(len(b))):
            z1, z0 = one.apply_precond(r), bj.apply_precond(r)
            scale = np.repeat(np.abs(z0).reshape(-1, 3).max(axis=1), 3)
            ulps = np.abs(z1 - z0) / np.spacing(scale)
            print(f"{name}: segment 1 against block-Jacobi, largest difference {ulps.max():.3g} ulp "
                  f"({'bit-identical' if np.array_equal(z1, z0) else 'not bit-identical'})")
            assert ulps.max() <= 4.0
    finally:
        one.close()
        bj.close()


def test_apply_precond_moves_nothing():
    dev = _dev("mixed72", ("chain", 16))
    try:
        assert dev.update()[0]
        before = (dev.get_poses(), dev.get_delta(), dev.timing(), dev.get_bsr()[2], dev.precond_info())
        z1 = dev.apply_precond(np.ones(3 * 72))
        z2 = dev.apply_precond(np.ones(3 * 72))
        np.testing.assert_array_equal(z1, z2)
        after = (dev.get_poses(), dev.get_delta(), dev.timing(), dev.get_bsr()[2], dev.precond_info())
        for u, v in zip(before, after):
            if isinstance(u, dict):
                assert u == v
            else:
                np.testing.assert_array_equal(u, v)
    finally:
        dev.close()


def test_dense_path_accepts_and_ignores_it():
    """n = 216 <= 2048 under solver="auto": the update is the default handle's bit
    for bit, and apply_precond factors on demand (no solve has done it)."""
    plain = _dev("mixed72", "untouched", solver="auto")
    chain = _dev("mixed72", ("chain", 8), solver="auto")
    try:
        assert plain.update() == chain.update()
        np.testing.assert_array_equal(plain.get_poses(), chain.get_poses())
        np.testing.assert_array_equal(plain.get_delta(), chain.get_delta())
        assert chain.timing()["pcg_iterations"] == 0
        M, nt, want = _m_of(chain, 8)
        r = np.random.RandomState(5).standard_normal(3 * nt)
        ref = np.linalg.solve(M, r)
        z = chain.apply_precond(r)
        assert np.abs(z - ref).max() <= np.linalg.cond(M) * 1e-12 * np.abs(ref).max()
        assert chain.precond_info() == dict(kind="chain", segment=8, off_diagonal_blocks=want, bad_pivots=0)
    finally:
        plain.close()
        chain.close()


# ------------------------------------------------------------------ 2. the solve
@pytest.mark.parametrize("T", [72, 300])
def test_solve_matches_restatement_and_block_jacobi(T):
    case = _table_case(T)
    H, b = cr.table_system(T, True)
    ref = -np.linalg.solve(H, b)
    out = {}
    for pre in ("block_jacobi", ("chain", 4), ("chain", 64)):
        dev = _dev(case, pre, pcg_tol=1e-12)
        try:
            st = dev.update()
            assert st[0], pre
            delta = dev.get_delta()
            gap = np.abs(delta - ref).max()
            print(f"T = {T} {pre}: delta gap {gap:.3g} (max |delta| {np.abs(ref).max():.3g}), "
                  f"{dev.timing()['pcg_iterations']} PCG iterations at tol 1e-12")
            assert gap <= 1e-6 * np.abs(ref).max(), pre
            stats = dev.optimize(0.01, 50)
            assert np.all(stats[:, 0] == 1.0)
            out[pre] = (1 + len(stats), dev.get_poses())
        finally:
            dev.close()
    n_bj, p_bj = out["block_jacobi"]
    for pre in (("chain", 4), ("chain", 64)):
        assert out[pre][0] == n_bj, (pre, out[pre][0], n_bj)
        np.testing.assert_allclose(out[pre][1], p_bj, rtol=0, atol=1e-8)


@pytest.mark.parametrize("T", [72, 300])
def test_iteration_counts_fall_with_the_segment(T):
    case = _table_case(T)
    counts = {}
    for S in (0, 1, 4, 16, 64):
        dev = _dev(case, "block_jacobi" if S == 0 else ("chain", S))
        try:
            assert dev.update()[0]
            counts[S] = dev.timing()["pcg_iterations"]
        finally:
            dev.close()
    cpu = {S: cr.table_iterations(T, True, S) for S in counts}
    print(f"T = {T}: device PCG iterations {counts}; restatement {cpu} "
          f"(block-Jacobi's own distance: {counts[0] - cpu[0]:+d})")
    assert counts[64] <= counts[16] <= counts[4] <= counts[0]
    assert 4 * counts[64] <= counts[0]


# ------------------------------------------------- 3. defaults and determinism
def test_block_jacobi_and_untouched_handles_are_bit_identical():
    case = _table_case(300)
    res = []
    for pre in ("untouched", "block_jacobi", None):
        dev = _dev(case, pre)
        try:
            st = dev.update()
            # det and cond are not formed on the PCG path (NaN): is_calc and sum delta^2
            res.append((st[:2], dev.get_delta(), dev.get_poses(), dev.timing()["pcg_iterations"]))
            stats = dev.optimize(0.01, 50)
            res[-1] += (stats, dev.get_poses())
        finally:
            dev.close()
    for other in res[1:]:
        assert other[0] == res[0][0] and other[3] == res[0][3]
        for k in (1, 2, 4, 5):
            np.testing.assert_array_equal(other[k], res[0][k])


def test_two_chain_runs_are_bit_identical():
    case = _table_case(300)
    res = []
    for _ in range(2):
        dev = _dev(case, ("chain", 64))
        try:
            st = dev.update()
            res.append((st[:2], dev.get_delta(), dev.timing()["pcg_iterations"], dev.optimize(0.01, 50),
                        dev.get_poses(), dev.apply_precond(np.arange(900.0))))
        finally:
            dev.close()
    assert res[0][0] == res[1][0] and res[0][2] == res[1][2]
    for k in (1, 3, 4, 5):
        np.testing.assert_array_equal(res[0][k], res[1][k])


def test_set_precond_takes_effect_at_the_next_linearisation():
    dev = _dev("mixed200", "untouched")
    try:
        assert dev.precond_info()["kind"] == "block_jacobi"
        assert dev.update()[0]
        n_bj = dev.timing()["pcg_iterations"]
        dev.set_precond("chain")                                  # segment 0 / None: 64
        assert dev.precond_info()["kind"] == "block_jacobi"       # still in force
        dev.set_poses(cr.case("mixed200")[0])
        assert dev.update()[0]
        assert dev.precond_info()["kind"] == "chain" and dev.precond_info()["segment"] == 64
        assert dev.timing()["pcg_iterations"] < n_bj
        dev.set_precond(None)
        dev.set_poses(cr.case("mixed200")[0])
        assert dev.update()[0]
        assert dev.precond_info()["kind"] == "block_jacobi"
        assert dev.timing()["pcg_iterations"] == n_bj
    finally:
        dev.close()


# ------------------------------------------------------------- 4. bad pivots
def test_nan_pose_gives_bad_pivots_and_no_update():
    """slam_graph_set_poses accepts non-finite poses: the factor counts the
    pivots they spoil and the solve ends before it forms any delta."""
    poses, rec, od, robust = cr.case("mixed200")
    bad = poses.copy()
    bad[70] = np.nan
    dev = _dev((bad, rec, od, robust), ("chain", 64))
    try:
        st = dev.update()
        assert st[0] is False and st[1] == 0.0
        info = dev.precond_info()
        assert info["kind"] == "chain" and info["bad_pivots"] > 0
        assert dev.timing()["pcg_iterations"] == 0
        np.testing.assert_array_equal(dev.get_poses(), bad)       # nothing moved
        # the handle recovers with finite poses
        dev.set_poses(poses)
        assert dev.update()[0] and dev.precond_info()["bad_pivots"] == 0
    finally:
        dev.close()


# ------------------------------------------ 5. argument errors, a real handle
def test_argument_errors_leave_the_handle():
    from slamhip import _lib
    twin = _dev("mixed72", ("chain", 16))
    dev = _dev("mixed72", ("chain", 16))
    lib = dev._lib
    try:
        # apply_precond before any assembly
        vec = np.ones(3 * 72)
        out = np.full(3 * 72, 7.0)
        assert lib.slam_graph_apply_precond(dev._h, _lib.dptr(vec), _lib.dptr(out)) == _lib.SLAM_ERR_ARG
        assert "no system assembled" in lib.slam_last_error().decode()
        assert np.all(out == 7.0)
        # bad segments and kinds
        for kind, seg in ((1, 3), (1, -1), (1, 65), (1, 128), (2, 64), (-1, 0)):
            assert lib.slam_graph_set_precond(dev._h, kind, seg) == _lib.SLAM_ERR_ARG
            assert "slam_graph_set_precond" in lib.slam_last_error().decode()
        assert dev.update()[:2] == twin.update()[:2]
        assert dev.precond_info() == twin.precond_info()
        assert dev.precond_info()["segment"] == 16
        np.testing.assert_array_equal(dev.get_delta(), twin.get_delta())
        np.testing.assert_array_equal(dev.apply_precond(vec), twin.apply_precond(vec))
        # a new edge set: nothing assembled again
        dev.set_edges(cr.case("mixed72")[1], odometry=cr.case("mixed72")[2])
        assert lib.slam_graph_apply_precond(dev._h, _lib.dptr(vec), _lib.dptr(out)) == _lib.SLAM_ERR_ARG
        # the segment is ignored for block-Jacobi
        assert lib.slam_graph_set_precond(dev._h, 0, 12345) == _lib.SLAM_OK
    finally:
        dev.close()
        twin.close()


# ------------------------------------------------------------- 6. front end
def test_trajectory_estimator_passes_it_through():
    import graph_odom_ref as gr
    from graph_based_slam import TrajectoryEstimator
    init, _, _, od = cr._circle(72, 5)
    poses = [p.reshape(3, 1).copy() for p in init[:30]]
    te = TrajectoryEstimator(poses[0], solver="pcg")
    te.setOdometry(gr.SIGMA)
    te.setPrecond(("chain", 16))
    for k in range(1, 30):
        te.addPose(poses[k], False, od["rel"][k - 1])
    assert te.updateEstPose()[0]
    assert te._dev.precond_info() == dict(kind="chain", segment=16, off_diagonal_blocks=28, bad_pivots=0)
