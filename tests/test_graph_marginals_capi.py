"""slam_graph_marginals / slam_graph_set_marginal_cols without a GPU: the
exports, their declarations and bindings, the NULL checks that come before any
HIP call, and the front-end methods' signatures."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from slamhip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slam_hip.h")
NAMES = ("slam_graph_marginals", "slam_graph_set_marginal_cols")


def test_exports_declared_and_bound():
    text = open(HEADER).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    res, args = _lib.SIGNATURES["slam_graph_marginals"]
    assert res is C.c_int and len(args) == 6 and args[1] is C.c_int64 and args[3] is C.c_int32
    # the contract is part of the header
    doc = text[text.index("Joint marginal covariance"):text.index("int slam_graph_set_marginal_cols")]
    for phrase in ("SLAM_ERR_ARG", "NaN", "NOT re-run", "not symmetrised", "relinearize = 0"):
        assert phrase in doc, phrase


def _err(rc):
    assert rc == _lib.SLAM_ERR_ARG
    msg = _lib.load().slam_last_error().decode()
    assert msg
    return msg


def test_null_arguments_are_argument_errors():
    lib = _lib.load()
    times = np.zeros(1, dtype=np.int64)
    cov = np.zeros((3, 3))
    info = np.zeros(6)
    tp = times.ctypes.data_as(C.POINTER(C.c_int64))
    assert "slam_graph_marginals" in _err(
        lib.slam_graph_marginals(None, 1, tp, 1, _lib.dptr(cov), _lib.dptr(info)))
    assert "slam_graph_set_marginal_cols" in _err(lib.slam_graph_set_marginal_cols(None, 0))
    # a non-NULL handle is never dereferenced before the pointer checks fail
    fake = C.c_void_p(C.addressof(C.create_string_buffer(8)))
    _err(lib.slam_graph_marginals(fake, 1, None, 1, _lib.dptr(cov), _lib.dptr(info)))
    _err(lib.slam_graph_marginals(fake, 1, tp, 1, None, _lib.dptr(info)))
    _err(lib.slam_graph_marginals(fake, 1, tp, 1, _lib.dptr(cov), None))
    _err(lib.slam_graph_marginals(fake, 0, tp, 1, _lib.dptr(cov), _lib.dptr(info)))
    assert np.all(cov == 0) and np.all(info == 0)


def test_front_end_methods():
    from graph_based_slam import Robot, TrajectoryEstimator
    from slamhip.graph import DeviceGraph
    p = inspect.signature(DeviceGraph.marginals).parameters
    assert list(p) == ["self", "times", "relinearize", "joint", "symmetrize"]
    assert (p["relinearize"].default, p["joint"].default, p["symmetrize"].default) == (True, False, True)
    assert list(inspect.signature(DeviceGraph.set_marginal_cols).parameters) == ["self", "cols"]
    p = inspect.signature(TrajectoryEstimator.getEstTrajCov).parameters
    assert list(p) == ["self", "times"] and p["times"].default is None
    assert list(inspect.signature(Robot.getEstTrajCov).parameters) == ["self"]
    p = inspect.signature(Robot.draw).parameters
    assert list(p) == ["self", "aAx1", "aAx2", "ellipses"] and p["ellipses"].default is False
