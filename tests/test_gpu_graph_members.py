"""Graph SLAM ensembles (slam_graph_set_members): member m of a
handle with members is bit for bit what a stand-alone handle with the same
configuration returns for member m's poses and edges alone -- the poses, every
stats row, the iteration count, delta, the assembled H and b and the edge
weights -- whatever the other members are, however many and in whatever order.

In every test the reference is a stand-alone DeviceGraph per member in the same
process (computed once per member and robust kind, shared, read-only), and
"equal" is np.array_equal (NaN equal to NaN where a member's own input is NaN).
The comparison with NumPy uses the bar of test_gpu_graph_odom.py's
test_gauss_newton_matches_restatement for the same comparison on a single
handle: the same iteration count, is_calc throughout, poses atol 1e-8."""
import ctypes as C
import functools

import numpy as np
import pytest

import graph_odom_ref as gr
import graph_robust_ref as rr

pytestmark = pytest.mark.gpu

MAX_ITER = 50
KW = dict(solver="dense")


def _robust(robust):
    return None if robust is None or robust[0] is None else robust


@functools.lru_cache(maxsize=None)
def member(name):
    """(poses, edges, odometry or None) with member-local indices, read-only."""
    from slamhip.graph import EDGE_DTYPE, circle_graph, circle_graph_odometry
    if name == "two":                                   # two poses with one edge
        init, _, rec = circle_graph(2, n_landmarks=16, seed=5)
        assert len(rec) >= 1
        out = (init, rec[:1].copy(), None)
    elif name in ("c72o", "c72"):                       # seed 5, 264 pairs, with / without odometry
        init, _, rec, _, _ = rr.corrupted_graph(5)
        out = (init, rec, gr.odometry(5) if name == "c72o" else None)
    elif name in ("cor5", "cor6"):                      # one pairing in ten wrong, with odometry
        seed = int(name[3:])
        init, _, _, cor, _ = rr.corrupted_graph(seed)
        out = (init, cor, gr.odometry(seed))
    elif name in ("c257", "c300", "c682"):              # the partial boundary of sum delta^2: 256 poses
        T = int(name[1:])
        # a start near the truth: few iterations of the one-workgroup dense kernels,
        # which take ~0.7 s per update at 900 unknowns and ~8 s at 2046 on either handle
        init, truth, rec = circle_graph(T, n_landmarks=64, seed=T, odom_noise=2e-4)
        out = (init, rec, circle_graph_odometry(truth, gr.SIGMA, T))
    elif name == "noedge":                              # poses but no edge
        out = (rr.corrupted_graph(6)[0][:3].copy(), np.zeros(0, dtype=EDGE_DTYPE), None)
    elif name == "late":                                # its first three poses are touched by no edge
        init, rec, od = member("c72o")
        rec, od = rec.copy(), od.copy()
        for r in (rec, od):
            for f in ("time_bfr", "pose_bfr", "time_aft", "pose_aft"):
                r[f] += 3
        out = (np.concatenate([init[:3] + 1.0, init]), rec, od)
    elif name == "singular":                            # test_gate_rejects_singular_h_on_both_paths' graph
        init, _, edges = circle_graph(300, n_landmarks=64, seed=0, odom_noise=0.002)
        keep = (edges["time_bfr"] < 150) == (edges["time_aft"] < 150)
        edges = edges[keep]
        assert (edges["time_bfr"] >= 150).any() and (edges["time_aft"] < 150).any()
        out = (init, edges, None)
    elif name == "nan":                                 # a NaN pose
        init, rec, od = member("c72o")
        init = init.copy()
        init[10, 0] = np.nan
        out = (init, rec, od)
    else:
        raise KeyError(name)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def _results(dev, robust):
    """What the contract covers, of a stand-alone handle after its last update."""
    out = dict(poses=dev.get_poses(), delta=dev.get_delta())
    if dev.n_edges:
        times, H, b, _ = dev.get_system(dense=True)
    else:                                               # no edge set: no system
        times, H, b = np.zeros(0, dtype=np.int64), np.zeros((0, 0)), np.zeros(0)
    out.update(times=times, H=H, b=b)
    if _robust(robust) is not None and len(times) > 1:
        out["weights"] = np.stack(dev.edge_weights())
    return out


@functools.lru_cache(maxsize=None)
def reference(name, robust=None, mode="optimize"):
    """The stand-alone handle of one member: stats, n_iter and _results."""
    from slamhip.graph import DeviceGraph
    poses, edges, od = member(name)
    dev = DeviceGraph(robust=_robust(robust), **KW)
    try:
        dev.set_poses(poses)
        dev.set_edges(edges, odometry=od)
        if mode == "optimize":
            st = dev.optimize(0.01, MAX_ITER)
        else:
            st = np.array([dev.update()], dtype=np.float64)
        out = dict(stats=st, **_results(dev, robust))
    finally:
        dev.close()
    for a in out.values():
        a.setflags(write=False)
    return out


def _ensemble(names, robust=None, mode="optimize"):
    return _ensemble_run(tuple(names), robust, mode)


@functools.lru_cache(maxsize=None)
def _ensemble_run(names, robust, mode):
    """The same members in one handle: per member what reference() returns
    (one run per list of members, shared by the tests, read-only)."""
    from slamhip.graph import DeviceGraphEnsemble
    ens = DeviceGraphEnsemble(robust=_robust(robust), **KW)
    try:
        ens.set_members([member(n) for n in names])
        if mode == "optimize":
            stats = ens.optimize(0.01, MAX_ITER)
        else:
            stats = [row[None, :] for row in ens.update()]
        poses, delta, system = ens.get_poses(), ens.get_delta(), ens.get_system()
        weights = ens.edge_weights() if _robust(robust) is not None else None
    finally:
        ens.close()
    out = []
    for m in range(len(names)):
        r = dict(stats=stats[m], poses=poses[m], delta=delta[m], times=system[m][0], H=system[m][1],
                 b=system[m][2])
        if weights is not None and len(r["times"]) > 1:
            r["weights"] = np.stack(weights[m])
        for a in r.values():
            a.setflags(write=False)
        out.append(r)
    return out


def _assert_member(got, ref, what):
    # delta is that of the last solved update: a member none of whose updates
    # passed the gate never had one written
    keys = ("stats", "poses", "times", "H", "b") + (("delta",) if ref["stats"][:, 0].any() else ())
    for k in keys + (("weights",) if "weights" in ref else ()):
        assert got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k], equal_nan=True), (what, k)


def _check(names, robust=None, mode="optimize"):
    got = _ensemble(names, robust, mode)
    for m, n in enumerate(names):
        _assert_member(got[m], reference(n, robust, mode), (m, n))
    return got


# ------------------------------------------------------------ 1. one member
@pytest.mark.parametrize("mode", ["update", "optimize"])
def test_one_member_is_the_plain_handle(mode):
    got = _check(["c72o"], mode=mode)
    assert got[0]["stats"][0, 0] == 1.0


# ------------------------------------------------- 2. unequal members together
CASE2 = ["two", "c72o", "c72", "c257", "noedge", "c300", "late"]


def test_unequal_members_stop_on_their_own_and_stay_frozen():
    """Members of 2 to 300 poses, one without an edge, one whose first poses no
    edge touches, stopping after different iteration counts: each equals its
    stand-alone handle after that handle's own last update (stats, n_iter,
    poses, delta, H, b), so an early stopper was left alone from then on."""
    got = _check(CASE2)
    n_iter = [len(g["stats"]) for g in got]
    print("iterations per member:", dict(zip(CASE2, n_iter)))
    assert n_iter[CASE2.index("c72o")] == 5 and n_iter[CASE2.index("c72")] == 36
    assert n_iter == [len(reference(n)["stats"]) for n in CASE2]
    assert len(set(n_iter)) >= 3                             # early and late stoppers stand together
    # the member without an edge: a zero row, as do_update returns, poses untouched
    g = got[CASE2.index("noedge")]
    assert np.array_equal(g["stats"], np.zeros((1, 4))) and len(g["times"]) == 0
    assert np.array_equal(g["poses"], member("noedge")[0])
    # the poses no edge touches stay; the member's times start behind them
    g = got[CASE2.index("late")]
    assert np.array_equal(g["poses"][:3], member("late")[0][:3]) and g["times"][0] == 3
    assert np.array_equal(g["poses"][3:], reference("c72o")["poses"])
    assert np.array_equal(g["stats"], reference("c72o")["stats"])


def test_update_of_unequal_members():
    _check(CASE2, mode="update")


# ----------------------------------------- 3. permuted, and one member repeated
def test_permuted_members_and_twenty_copies():
    order = ["late", "c300", "c72", "noedge", "two", "c257", "c72o"]
    assert sorted(order) == sorted(CASE2) and order != CASE2
    _check(order)
    got = _check(["c72o"] * 20)
    for g in got[1:]:
        _assert_member(g, got[0], "copy")


# --------------------------------------------------------------- 4. robust kinds
@pytest.mark.parametrize("robust", [("cauchy", 2.0), ("dcs", 5.0)], ids=["cauchy2", "dcs5"])
def test_robust_kinds(robust):
    got = _check(["cor5", "cor6"], robust=robust)
    for g in got:
        assert g["weights"].shape[0] == 2 and (g["weights"][1] < 0.1).any()   # wrong pairings rejected


# ----------------------------------------------------------- 5. singular, NaN
def test_singular_member_among_healthy_ones():
    names = ["c72o", "singular", "c72"]
    got = _check(names)
    g = got[1]
    assert len(g["stats"]) == 1 and g["stats"][0, 0] == 0.0 and g["stats"][0, 1] == 0.0
    assert not (g["stats"][0, 3] < 1e15)
    assert np.array_equal(g["poses"], member("singular")[0])


def test_member_with_a_nan_pose():
    names = ["c72o", "nan", "two"]
    got = _check(names)
    ref = reference("nan")
    assert np.array_equal(got[1]["stats"], ref["stats"], equal_nan=True)
    assert ref["stats"][-1, 0] == 0.0                          # NaN passes no gate


# -------------------------------------------------------------- 6. against NumPy
def test_members_match_the_numpy_restatement():
    names = [n for n in CASE2 if len(member(n)[0]) <= 75 and n != "noedge"]
    assert names == ["two", "c72o", "c72", "late"]
    got = _ensemble(CASE2)
    for n in names:
        poses, edges, od = member(n)
        if n in ("c72o", "c72"):
            ref_p, ref_st = gr.cpu_run(5, None, None, False, n == "c72o")
        else:
            ref_p, ref_st = gr.gauss_newton(rr.edge_rows(edges).reshape(len(edges), 11),
                                            gr.odom_rows(od) if od is not None else np.empty((0, 10)),
                                            poses, max_iter=MAX_ITER)
        g = got[CASE2.index(n)]
        print(f"{n}: {len(g['stats'])} iterations, gap to the restatement "
              f"{np.abs(g['poses'] - ref_p).max():.3g}")
        assert len(g["stats"]) == len(ref_st) and np.all(g["stats"][:, 0] == 1.0)
        np.testing.assert_allclose(g["poses"], ref_p, rtol=0, atol=1e-8)


# --------------------------------------------------------- 7. the largest member
def test_largest_member_and_one_pose_more():
    from slamhip._lib import SLAM_ERR_ARG, SlamError
    from slamhip.graph import DeviceGraphEnsemble
    assert len(member("c682")[0]) == 682
    _check(["c682", "two"], mode="update")
    ens = DeviceGraphEnsemble(**KW)
    try:
        with pytest.raises(SlamError) as e:
            ens.set_members([(np.zeros((683, 3)), [], None)])
        assert e.value.code == SLAM_ERR_ARG and "682" in str(e.value)
    finally:
        ens.close()


# ------------------------------------------------- 8. argument checks, real handle
def _raw_members(ens, names):
    """The union's arrays as DeviceGraphEnsemble.set_members forms them."""
    poses = np.concatenate([member(n)[0] for n in names])
    off = np.concatenate([[0], np.cumsum([len(member(n)[0]) for n in names])]).astype(np.int64)
    return poses, off


def test_argument_checks_leave_the_handle():
    from slamhip import _lib
    from slamhip.graph import DeviceGraph, DeviceGraphEnsemble, EDGE_DTYPE
    lib = _lib.load()
    names = ["two", "c72o"]
    P64 = C.POINTER(C.c_int64)

    def bad(rc, text):
        assert rc == _lib.SLAM_ERR_ARG
        assert text in lib.slam_last_error().decode(), lib.slam_last_error().decode()

    def good(ens):
        """a following valid call gives the reference's bits"""
        st = ens.optimize(0.01, MAX_ITER)
        poses = ens.get_poses()
        for m, n in enumerate(names):
            assert np.array_equal(st[m], reference(n)["stats"]), n
            assert np.array_equal(poses[m], reference(n)["poses"]), n

    ens = DeviceGraphEnsemble(**KW)
    try:
        h = ens._dev._h
        st = np.zeros((2, 4))
        # update_members without members
        bad(lib.slam_graph_update_members(h, _lib.dptr(st)), "no members")
        ens.set_members([member(n) for n in names])
        # offsets that do not increase, do not start at 0, do not end at the pose count
        for off in ([0, 2, 2, 74], [0, 80, 74], [1, 2, 74], [0, 2, 73]):
            off = np.array(off, dtype=np.int64)
            rc = lib.slam_graph_set_members(h, len(off) - 1, off.ctypes.data_as(P64))
            bad(rc, "offsets")
        # an edge across two members; a time outside its member
        _, rec, _ = member("c72o")
        for field, value in (("pose_aft", 1), ("time_aft", 0)):
            e = rec[:4].copy()
            for f in ("time_bfr", "pose_bfr", "time_aft", "pose_aft"):
                e[f] += 2
            e[field][2] = value
            bad(lib.slam_graph_set_edges(h, len(e), e.ctypes.data_as(C.c_void_p)), "not in one member")
        # update() and optimize() on a handle with members
        one = np.zeros(4)
        bad(lib.slam_graph_update(h, _lib.dptr(one)), "has members")
        n = C.c_int32(0)
        bad(lib.slam_graph_optimize(h, 0.01, 5, None, C.byref(n)), "has members")
        t = np.zeros(1, dtype=np.int64)
        cov, info = np.zeros((3, 3)), np.zeros(6)
        bad(lib.slam_graph_marginals(h, 1, t.ctypes.data_as(P64), 1, _lib.dptr(cov), _lib.dptr(info)),
            "members")
        vec = np.zeros(3 * 74)
        bad(lib.slam_graph_apply_precond(h, _lib.dptr(vec), _lib.dptr(vec.copy())), "members")
        good(ens)                                             # the handle is as set_members left it
        # n_members = 0 returns the handle to the plain form (with no edge set)
        assert lib.slam_graph_set_members(h, 0, None) == _lib.SLAM_OK
        bad(lib.slam_graph_update_members(h, _lib.dptr(st)), "no members")
        assert ens._dev.update() == (False, 0.0, 0.0, 0.0)
    finally:
        ens.close()
    # solver="pcg"
    ens = DeviceGraphEnsemble(solver="pcg")
    try:
        with pytest.raises(_lib.SlamError) as e:
            ens.set_members([member(n) for n in names])
        assert e.value.code == _lib.SLAM_ERR_ARG and "PCG" in str(e.value)
    finally:
        ens.close()


# ------------------------------------------------------ 9. estimate_trajectories
def _robot(steps, odometry, seed):
    import graph_based_slam as gs
    np.random.seed(seed)
    x0 = np.array([[10.0], [0.0], [np.deg2rad(90.0)]])
    rbt = gs.Robot(x0, gs.PERIOD_ms / 1000, gs.SCN_SENS_RANGE_m, gs.SCN_SENS_ANGLE_rps, gs.LAND_MARKS)
    if odometry is not None:
        rbt.setOdometry(odometry)
    for _ in range(steps):
        rbt.move(gs.VEL_mps, gs.OMEGA_rps)
    return rbt


def test_estimate_trajectories_matches_each_estimator():
    import graph_based_slam as gs
    fleet = [(12, None, 7), (12, (0.05, 0.05, 0.02), 8), (8, None, 9)]
    alone = [_robot(*f) for f in fleet]
    ref_st = [r._est.estimate_trajectory(r._halves, r._sensor.getLandMarkNum(), 30) for r in alone]
    together = [_robot(*f) for f in fleet]
    st = gs.estimate_trajectories([r._est for r in together], [r._halves for r in together],
                                  [r._sensor.getLandMarkNum() for r in together], max_iter=30)
    for a, b, sa, sb in zip(alone, together, ref_st, st):
        assert np.array_equal(sa, sb)
        pa = np.array([p[:, 0] for p in a._est._poses])
        pb = np.array([p[:, 0] for p in b._est._poses])
        assert np.array_equal(pa, pb)
        assert b._est._rows == [] and b._est._times == [] and len(b._est._pairs) == len(a._est._pairs)
    assert all(s[0, 0] == 1.0 for s in st)


# ------------------------------------------------------------ 10. the plain handle
def test_plain_handle_is_unchanged_by_a_members_episode():
    """A handle that held members and was returned to the plain form gives the
    results of a handle that never held any."""
    from slamhip.graph import DeviceGraphEnsemble
    ref = reference("c72o")
    ens = DeviceGraphEnsemble(**KW)
    try:
        ens.set_members([member("c300"), member("two")])
        ens.update()
        dev = ens._dev                                        # set_poses clears the members
        poses, edges, od = member("c72o")
        dev.set_poses(poses)
        dev.set_edges(edges, odometry=od)
        st = dev.optimize(0.01, MAX_ITER)
        assert np.array_equal(st, ref["stats"]) and np.array_equal(dev.get_poses(), ref["poses"])
        _, H, b, _ = dev.get_system(dense=True)
        assert np.array_equal(H, ref["H"]) and np.array_equal(b, ref["b"])
    finally:
        ens.close()
