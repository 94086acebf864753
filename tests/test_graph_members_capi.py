"""The members' entry points (slam_graph_set_members, slam_graph_update_members,
slam_graph_optimize_members) without a GPU: the exports, their
declarations, bindings and the contract in the header, the argument checks that
come before any HIP call, and the front ends' signatures.  The checks that need a
real handle are in test_gpu_graph_members.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from slamhip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slam_hip.h")
P, D = C.c_void_p, C.POINTER(C.c_double)
I64, I32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
EXPORTS = {"slam_graph_set_members": (C.c_int, [P, C.c_int64, I64]),
           "slam_graph_update_members": (C.c_int, [P, D]),
           "slam_graph_optimize_members": (C.c_int, [P, C.c_double, C.c_int32, D, I32])}


def test_exports_declared_bound_and_documented():
    text = open(HEADER).read()
    lib = _lib.load()
    for name, sig in EXPORTS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name) and _lib.SIGNATURES[name] == sig, name
        fn = getattr(lib, name)
        assert fn.restype == sig[0] and list(fn.argtypes) == sig[1], name
    doc = text[text.index("Members (DESIGN 8.6"):text.index("int slam_graph_set_members")]
    doc = " ".join(doc.replace("\n *", " ").split())          # the comment's words, line breaks aside
    for phrase in ("disjoint contiguous ranges", "bit for bit", "stand-alone", "its own anchor",
                   "pose_off[0] = 0", "increase strictly", "682 poses", "SLAM_GRAPH_PCG",
                   "n_members = 0 returns the handle to the plain form", "clears the edge set",
                   "in one member's range", "SLAM_ERR_ARG", "before any HIP call",
                   "leaves the handle as it was", "slam_graph_marginals", "slam_graph_apply_precond",
                   "zero row", "is_calc = 0 in a member is not an error",
                   "nothing it owns is written", "rows beyond n_iter[m] zero"):
        assert phrase in doc, phrase
    assert C.sizeof(_lib.GraphConfig) == 80                   # slam_graph_config keeps its layout


def _err(rc, name):
    assert rc == _lib.SLAM_ERR_ARG
    msg = _lib.load().slam_last_error().decode()
    assert name in msg, msg
    return msg


def test_argument_errors_before_any_hip_call():
    lib = _lib.load()
    st = np.full(8, 7.0)
    it = np.full(2, 7, dtype=np.int32)
    off = np.array([0, 1], dtype=np.int64)
    dp = lambda a: a.ctypes.data_as(D)
    ip = lambda a: a.ctypes.data_as(I32)
    op = lambda a: a.ctypes.data_as(I64)
    assert "NULL handle" in _err(lib.slam_graph_set_members(None, 1, op(off)), "slam_graph_set_members")
    assert "NULL" in _err(lib.slam_graph_update_members(None, dp(st)), "slam_graph_update_members")
    _err(lib.slam_graph_optimize_members(None, 0.01, 5, dp(st), ip(it)), "slam_graph_optimize_members")
    # an all-zero block far larger than the handle: a handle with no poses and no
    # members; the checks read it and write nothing
    zero = C.create_string_buffer(1 << 16)
    blank = C.c_void_p(C.addressof(zero))
    assert "NULL offsets" in _err(lib.slam_graph_set_members(blank, 1, None), "slam_graph_set_members")
    assert "negative" in _err(lib.slam_graph_set_members(blank, -1, op(off)), "slam_graph_set_members")
    assert "set the poses first" in _err(lib.slam_graph_set_members(blank, 1, op(off)),
                                         "slam_graph_set_members")
    assert "NULL" in _err(lib.slam_graph_update_members(blank, None), "slam_graph_update_members")
    assert "no members" in _err(lib.slam_graph_update_members(blank, dp(st)), "slam_graph_update_members")
    _err(lib.slam_graph_optimize_members(blank, 0.01, 5, dp(st), None), "slam_graph_optimize_members")
    _err(lib.slam_graph_optimize_members(blank, 0.01, 0, dp(st), ip(it)), "slam_graph_optimize_members")
    assert "no members" in _err(lib.slam_graph_optimize_members(blank, 0.01, 5, None, ip(it)),
                                "slam_graph_optimize_members")
    assert zero.raw == bytes(1 << 16)
    assert np.all(st == 7.0) and np.all(it == 7)              # no output was written


def test_front_end_signatures():
    import graph_based_slam as gbs
    from slamhip.graph import DeviceGraph, DeviceGraphEnsemble
    E = DeviceGraphEnsemble
    p = inspect.signature(E.__init__).parameters
    assert list(p) == ["self", "kwargs"] and p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(E.set_members).parameters) == ["self", "members"]
    assert list(inspect.signature(E.update).parameters) == ["self"]
    p = inspect.signature(E.optimize).parameters
    assert list(p) == ["self", "delta_sum_th", "max_iter"]
    assert p["delta_sum_th"].default == 0.01 and p["max_iter"].default == 100
    for name in ("get_poses", "get_delta", "edge_weights", "get_system", "close"):
        assert list(inspect.signature(getattr(E, name)).parameters) == ["self"], name
    p = inspect.signature(E.set_robust).parameters
    assert list(p) == ["self", "kind", "param"] and p["param"].default is None
    p = inspect.signature(gbs.estimate_trajectories).parameters
    assert list(p) == ["estimators", "halves", "n_landmarks", "max_iter"] and p["max_iter"].default == 100
    # the pinned constructors are unchanged
    assert list(inspect.signature(DeviceGraph.__init__).parameters) == [
        "self", "r_dist", "r_dir", "r_orient", "anchor", "det_min", "cond_max", "solver", "pcg_tol",
        "pcg_max_iter", "cond", "cond_tol", "cond_max_iter", "device", "robust"]
    assert list(inspect.signature(gbs.TrajectoryEstimator.__init__).parameters) == [
        "self", "aPose", "solver", "device", "robust"]
    assert list(inspect.signature(gbs.TrajectoryEstimator.estimate_trajectory).parameters) == [
        "self", "halves", "n_landmarks", "max_iter"]
    assert list(inspect.signature(gbs.Robot.__init__).parameters) == [
        "self", "aPose", "aDt", "aScanRng_m", "aScanAng_rad", "aLandMarks", "device", "robust"]


def test_estimate_trajectories_argument_errors_need_no_device():
    import graph_based_slam as gbs

    class Est:                                                # the fields the checks read
        def __init__(self, solver="auto", device=0, robust=None, rows=(), n_poses=3):
            self._solver, self._device, self._robust = solver, device, robust
            self._rows, self._poses = list(rows), [None] * n_poses

    def raises(ests, text):
        try:
            gbs.estimate_trajectories(ests, [[] for _ in ests], 4)
        except ValueError as e:
            assert text in str(e), e
        else:
            raise AssertionError(text)

    raises([Est(), Est(rows=[[0] * 10])], "pending")
    raises([Est(), Est(solver="dense")], "differ")
    raises([Est(), Est(device=1)], "differ")
    raises([Est(robust=("cauchy", 2.0)), Est(robust=("cauchy", 1.0))], "differ")
    raises([Est(), Est(n_poses=683)], "682")
