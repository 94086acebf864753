"""slam_graph_set_edges_odom without a GPU: the export, its declaration and
binding, the record layout, the argument checks that come before the handle is
read (and the one that reads only its pose pointer), and the front ends' new
signatures.  The checks of the records' contents -- index out of range,
time_bfr == time_aft, a non-finite rel, a sigma that is not finite and > 0 --
need a handle with poses, which needs the device: test_gpu_graph_odom.py runs
them on a real handle and shows that handle untouched."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from slamhip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slam_hip.h")
NAME = "slam_graph_set_edges_odom"


def test_export_declared_bound_and_documented():
    text = open(HEADER).read()
    lib = _lib.load()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, text)
    assert hasattr(lib, NAME) and NAME in _lib.SIGNATURES
    P = C.c_void_p
    assert _lib.SIGNATURES[NAME] == (C.c_int, [P, C.c_int64, P, C.c_int64, P])
    # the record's layout
    assert re.search(r"int64_t time_bfr, pose_bfr, time_aft, pose_aft;[^}]*double rel\[3\];\s*"
                     r"double sigma\[3\];\s*}\s*slam_graph_odom;", text)
    # the contract is part of the header
    doc = text[text.index("Odometry edges (DESIGN 8.4"):text.index("int %s" % NAME)]
    for phrase in ("landmark edges first", "never down-weighted", "w = 1 and rho = chi2", "SLAM_ERR_ARG",
                   "before any HIP call", "time_bfr == time_aft", "non-finite rel", "finite and > 0",
                   "slam_graph_set_edges_odom(h, n, e, 0, NULL)", "all E columns", "index prefix"):
        assert phrase in doc, phrase
    # the index space is stated where the per-edge outputs are declared
    for entry in ("slam_graph_get_system", "slam_graph_chi2", "slam_graph_get_edge_weights"):
        head = text[:text.index("int %s(" % entry)]
        assert "all E columns" in head[head.rindex("/*"):], entry
    # slam_graph_config keeps its layout: no new field
    assert C.sizeof(_lib.GraphConfig) == 80


def test_record_layout():
    from slamhip.graph import EDGE_DTYPE, ODOM_DTYPE, odom_array
    assert ODOM_DTYPE.itemsize == 80 == EDGE_DTYPE.itemsize
    names = ("time_bfr", "pose_bfr", "time_aft", "pose_aft", "rel", "sigma")
    assert ODOM_DTYPE.names == names
    assert [ODOM_DTYPE.fields[n][1] for n in names] == [0, 8, 16, 24, 32, 56]
    for n in names[:4]:                                     # the shared index prefix
        assert ODOM_DTYPE.fields[n] == EDGE_DTYPE.fields[n]
    rec = odom_array([[3, 4, 7, 8, 0.1, 0.2, 0.3, 0.02, 0.03, 0.01]])
    assert rec.dtype == ODOM_DTYPE and len(rec) == 1
    assert (rec["time_bfr"][0], rec["pose_bfr"][0], rec["time_aft"][0], rec["pose_aft"][0]) == (3, 4, 7, 8)
    np.testing.assert_array_equal(rec["rel"][0], [0.1, 0.2, 0.3])
    np.testing.assert_array_equal(rec["sigma"][0], [0.02, 0.03, 0.01])
    assert len(odom_array(np.empty((0, 10)))) == 0


def _err(rc):
    assert rc == _lib.SLAM_ERR_ARG
    msg = _lib.load().slam_last_error().decode()
    assert NAME in msg, msg
    return msg


def test_argument_errors_before_the_handle_is_read():
    from slamhip.graph import EDGE_DTYPE, ODOM_DTYPE
    lib = _lib.load()
    edges = np.zeros(2, dtype=EDGE_DTYPE)
    odom = np.zeros(2, dtype=ODOM_DTYPE)
    odom["sigma"] = 1.0
    ep, op = edges.ctypes.data_as(C.c_void_p), odom.ctypes.data_as(C.c_void_p)
    assert "NULL handle" in _err(lib.slam_graph_set_edges_odom(None, 2, ep, 2, op))
    # a non-NULL handle is not dereferenced before the counts and pointers are checked:
    # eight bytes of a pattern that no check may read or write
    buf = C.create_string_buffer(b"\x5a" * 8, 8)
    fake = C.c_void_p(C.addressof(buf))
    assert "negative count" in _err(lib.slam_graph_set_edges_odom(fake, -1, ep, 2, op))
    assert "negative count" in _err(lib.slam_graph_set_edges_odom(fake, 2, ep, -1, op))
    assert "NULL array" in _err(lib.slam_graph_set_edges_odom(fake, 2, None, 2, op))
    assert "NULL array" in _err(lib.slam_graph_set_edges_odom(fake, 2, ep, 2, None))
    assert "NULL array" in _err(lib.slam_graph_set_edges_odom(fake, 0, None, 1, None))
    assert buf.raw == b"\x5a" * 8
    # poses not set: the one check that reads the handle, and only its pose pointer
    # (NULL in an all-zero block far larger than the handle)
    zero = C.create_string_buffer(1 << 16)
    blank = C.c_void_p(C.addressof(zero))
    assert "poses first" in _err(lib.slam_graph_set_edges_odom(blank, 2, ep, 2, op))
    assert "poses first" in _err(lib.slam_graph_set_edges_odom(blank, 0, None, 0, None))
    assert zero.raw == bytes(1 << 16)
    assert not edges.view(np.uint8).any()                   # the inputs are inputs


def test_front_end_signatures():
    from graph_based_slam import Robot, TrajectoryEstimator
    from slamhip import graph
    from slamhip.graph import DeviceGraph
    p = inspect.signature(DeviceGraph.set_edges).parameters
    assert list(p) == ["self", "edges", "odometry"] and p["odometry"].default is None
    assert list(inspect.signature(graph.odom_array).parameters) == ["rows"]
    assert list(inspect.signature(graph.relpose).parameters) == ["xb", "xa"]
    assert list(inspect.signature(graph.circle_graph_odometry).parameters) == ["truth", "sigma", "seed"]
    assert list(inspect.signature(TrajectoryEstimator.setOdometry).parameters) == ["self", "sigma"]
    p = inspect.signature(TrajectoryEstimator.addPose).parameters
    assert list(p) == ["self", "aPose", "aIsObs", "aOdom"] and p["aOdom"].default is None
    assert list(inspect.signature(Robot.setOdometry).parameters) == ["self", "sigma"]
    # the pinned constructors are unchanged: no new keyword
    p = inspect.signature(DeviceGraph.__init__).parameters
    assert list(p) == ["self", "r_dist", "r_dir", "r_orient", "anchor", "det_min", "cond_max", "solver",
                       "pcg_tol", "pcg_max_iter", "cond", "cond_tol", "cond_max_iter", "device", "robust"]
    p = inspect.signature(TrajectoryEstimator.__init__).parameters
    assert list(p) == ["self", "aPose", "solver", "device", "robust"]
    p = inspect.signature(Robot.__init__).parameters
    assert list(p) == ["self", "aPose", "aDt", "aScanRng_m", "aScanAng_rad", "aLandMarks", "device",
                       "robust"]


def test_circle_graph_odometry_recipe():
    """One edge per consecutive pose pair, k-1 -> k, rel = relpose(truth) + sigma
    * RandomState(1000 + seed) normals drawn three per edge in order."""
    from slamhip.graph import ODOM_DTYPE, circle_graph, circle_graph_odometry, relpose
    _, truth, _ = circle_graph(72, n_landmarks=16, seed=5)
    sigma = (0.02, 0.02, 0.01)
    rec = circle_graph_odometry(truth, sigma, 5)
    assert rec.dtype == ODOM_DTYPE and len(rec) == 71
    np.testing.assert_array_equal(rec["time_bfr"], np.arange(71))
    np.testing.assert_array_equal(rec["pose_bfr"], np.arange(71))
    np.testing.assert_array_equal(rec["time_aft"], np.arange(1, 72))
    np.testing.assert_array_equal(rec["pose_aft"], np.arange(1, 72))
    noise = np.random.RandomState(1005).standard_normal((71, 3))
    want = np.array([relpose(truth[k - 1], truth[k]) for k in range(1, 72)]) + np.array(sigma) * noise
    np.testing.assert_array_equal(rec["rel"], want)
    np.testing.assert_array_equal(rec["sigma"], np.tile(sigma, (71, 1)))
    # every step of the circle is the same commanded motion: 10 m radius, 10 degrees
    step = 2 * 10 * np.sin(np.deg2rad(5.0))
    np.testing.assert_allclose(np.hypot(want[:, 0], want[:, 1]), step, atol=0.1)
