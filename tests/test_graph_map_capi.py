"""The landmark map's entry points without a GPU: the exports, their
declarations and bindings, the contract in the header, the argument checks that
come before the handle is read (and those that read only a field of an
all-zero block), and the front ends' signatures.  The checks of the records'
contents -- a pose index out of range, a non-finite observation, d <= 0 -- and
the refusal of a handle with members need a handle with poses, which needs the
device: test_gpu_graph_map.py runs them on a real handle and shows it untouched."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from slamhip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slam_hip.h")
P, D, I64 = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)
EXPORTS = {
    "slam_graph_set_observations": (C.c_int, [P, C.c_int64, P, C.c_int64]),
    "slam_graph_landmarks": (C.c_int, [P, D, D, I64, D, D]),
    "slam_graph_map_timing": (C.c_int, [P, D]),
}


def test_exports_declared_bound_and_documented():
    text = open(HEADER).read()
    lib = _lib.load()
    for name, sig in EXPORTS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name) and _lib.SIGNATURES[name] == sig, name
    assert re.search(r"int slam_graph_set_observations\(slam_graph\* h, int64_t n_halves,\s*"
                     r"const slam_graph_half\* halves,\s*int64_t n_landmarks\);", text)
    assert re.search(r"int slam_graph_landmarks\(slam_graph\* h, double\* mean[^,]*, double\* cov[^,]*,\s*"
                     r"int64_t\* count[^,]*, double\* chi2[^,]*,\s*double\* half_chi2[^)]*\);", text)
    doc = text[text.index("The landmark map of the trajectory (DESIGN 8.7"):
               text.index("int slam_graph_set_observations")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)                  # the comment's line breaks
    for phrase in ("information-weighted", "orientation does not enter", "uncertainty of the poses is NOT in it",
                   "robust kind does not enter", "chi2 = 0 exactly", "NaN mean, cov and chi2",
                   "no floating-point atomics", "bit-identical from call to call", "is ignored",
                   "half_chi2 comes back NaN", "n_halves = 0 clears", "different pose count",
                   "SLAM_ERR_ARG", "before any HIP call", "has members", "non-finite observation",
                   "distance <= 0", "any output may be NULL", "moves no pose", "allocates nothing"):
        assert phrase in doc, phrase
    assert C.sizeof(_lib.GraphConfig) == 80                 # slam_graph_config keeps its layout


def _err(rc, name):
    assert rc == _lib.SLAM_ERR_ARG
    msg = _lib.load().slam_last_error().decode()
    assert name in msg, msg
    return msg


def test_argument_errors_decided_on_the_host():
    from slamhip.graph import HALF_DTYPE
    lib = _lib.load()
    name = "slam_graph_set_observations"
    assert HALF_DTYPE.itemsize == 48
    halves = np.zeros(2, dtype=HALF_DTYPE)
    halves["obs"] = 1.0
    hp = halves.ctypes.data_as(C.c_void_p)
    assert "NULL handle" in _err(lib.slam_graph_set_observations(None, 2, hp, 1), name)
    # a non-NULL handle is not dereferenced before the counts and the pointer are
    # checked: eight bytes of a pattern that no check may read or write
    buf = C.create_string_buffer(b"\x5a" * 8, 8)
    fake = C.c_void_p(C.addressof(buf))
    assert "negative count" in _err(lib.slam_graph_set_observations(fake, -1, hp, 1), name)
    assert "negative count" in _err(lib.slam_graph_set_observations(fake, 2, hp, -1), name)
    assert "NULL array" in _err(lib.slam_graph_set_observations(fake, 2, None, 1), name)
    assert buf.raw == b"\x5a" * 8
    # poses not set: read from an all-zero block far larger than the handle
    zero = C.create_string_buffer(1 << 16)
    blank = C.c_void_p(C.addressof(zero))
    assert "poses first" in _err(lib.slam_graph_set_observations(blank, 2, hp, 1), name)
    assert "poses first" in _err(lib.slam_graph_set_observations(blank, 0, None, 0), name)
    # no observations: the same block has none
    out = np.zeros(8)
    dp = out.ctypes.data_as(D)
    assert "NULL handle" in _err(lib.slam_graph_landmarks(None, dp, None, None, None, None),
                                 "slam_graph_landmarks")
    assert "no observations" in _err(lib.slam_graph_landmarks(blank, dp, None, None, None, None),
                                     "slam_graph_landmarks")
    assert "no observations" in _err(lib.slam_graph_landmarks(blank, None, None, None, None, None),
                                     "slam_graph_landmarks")
    _err(lib.slam_graph_map_timing(None, dp), "slam_graph_map_timing")
    _err(lib.slam_graph_map_timing(blank, None), "slam_graph_map_timing")
    assert zero.raw == bytes(1 << 16) and not out.any()
    np.testing.assert_array_equal(halves["obs"], 1.0)       # the inputs are inputs


def test_front_end_signatures():
    from graph_based_slam import Robot, TrajectoryEstimator
    from slamhip import graph
    from slamhip.graph import DeviceGraph
    assert list(inspect.signature(DeviceGraph.set_observations).parameters) == ["self", "halves",
                                                                                "n_landmarks"]
    p = inspect.signature(DeviceGraph.landmarks).parameters
    assert list(p) == ["self", "per_observation"] and p["per_observation"].default is False
    assert list(inspect.signature(TrajectoryEstimator.getEstLandMarks).parameters) == ["self"]
    assert list(inspect.signature(Robot.getEstLandMarks).parameters) == ["self"]
    assert list(inspect.signature(Robot.drawEstLandMarks).parameters) == ["self", "ax"]
    assert list(inspect.signature(graph.circle_graph_halves).parameters) == ["n_poses", "n_landmarks", "seed",
                                                                             "odom_noise"]
    # the pinned constructors get no new keyword
    p = inspect.signature(DeviceGraph.__init__).parameters
    assert list(p) == ["self", "r_dist", "r_dir", "r_orient", "anchor", "det_min", "cond_max", "solver",
                       "pcg_tol", "pcg_max_iter", "cond", "cond_tol", "cond_max_iter", "device", "robust"]
    assert list(inspect.signature(TrajectoryEstimator.__init__).parameters) == ["self", "aPose", "solver",
                                                                                "device", "robust"]
    assert list(inspect.signature(Robot.__init__).parameters) == [
        "self", "aPose", "aDt", "aScanRng_m", "aScanAng_rad", "aLandMarks", "device", "robust"]


def test_circle_graph_halves_shares_circle_graph_world():
    """Every visible landmark a half-edge, by pose then by landmark id, from the
    same draws as circle_graph: its pair edges' observations are among them."""
    from slamhip.graph import HALF_DTYPE, circle_graph, circle_graph_halves
    init, truth, rec = circle_graph(40, n_landmarks=8, seed=3)
    _, truth2, halves, lm = circle_graph_halves(40, n_landmarks=8, seed=3)
    np.testing.assert_array_equal(truth, truth2)
    assert halves.dtype == HALF_DTYPE and lm.shape == (8, 2)
    np.testing.assert_array_equal(halves["time"], halves["pose"])
    key = halves["time"] * 8 + halves["landmark"]
    assert np.all(np.diff(key) > 0)
    np.testing.assert_allclose(np.hypot(lm[:, 0], lm[:, 1]), 14.0, rtol=1e-15)
    seen = {(int(t), *o) for t, o in zip(halves["time"], halves["obs"])}
    for e in rec:
        assert (int(e["time_bfr"]), *e["obs_bfr"]) in seen and (int(e["time_aft"]), *e["obs_aft"]) in seen
