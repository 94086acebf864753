"""slam_graph_set_robust / slam_graph_chi2 / slam_graph_get_edge_weights without
a GPU: the exports, their declarations and bindings, the argument checks that
come before any HIP call (outputs untouched), and the front ends' keywords."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from slamhip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slam_hip.h")
NAMES = ("slam_graph_set_robust", "slam_graph_chi2", "slam_graph_get_edge_weights")


def test_exports_declared_and_bound():
    text = open(HEADER).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    D = C.POINTER(C.c_double)
    assert _lib.SIGNATURES["slam_graph_set_robust"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_double])
    assert _lib.SIGNATURES["slam_graph_chi2"] == (C.c_int, [C.c_void_p, D, D, D])
    assert _lib.SIGNATURES["slam_graph_get_edge_weights"] == (C.c_int, [C.c_void_p, D, D])
    # the enums of the header are the binding's table
    for name, val in _lib.GRAPH_ROBUST.items():
        assert re.search(r"SLAM_GRAPH_ROBUST_%s\s*=\s*%d\b" % (name.upper(), val), text), name
    # the contract is part of the header
    doc = text[text.index("Robust edge weights"):text.index("int slam_graph_get_edge_weights")]
    for phrase in ("SLAM_ERR_ARG", "chi2 = 0 gives w = 1", "bit for bit", "WEIGHTED H",
                   "next linearisation", "fixed", "kind none", "w < 0.1"):
        assert phrase in doc, phrase
    # slam_graph_config keeps its layout
    assert C.sizeof(_lib.GraphConfig) == 80


def _err(rc):
    assert rc == _lib.SLAM_ERR_ARG
    msg = _lib.load().slam_last_error().decode()
    assert msg
    return msg


def test_argument_errors_leave_the_outputs():
    lib = _lib.load()
    tot = np.full(4, 7.0)
    c = np.full(3, 7.0)
    w = np.full(3, 7.0)
    assert "slam_graph_set_robust" in _err(lib.slam_graph_set_robust(None, 1, 1.0))
    assert "slam_graph_chi2" in _err(lib.slam_graph_chi2(None, _lib.dptr(tot), _lib.dptr(c), _lib.dptr(w)))
    assert "slam_graph_get_edge_weights" in _err(
        lib.slam_graph_get_edge_weights(None, _lib.dptr(c), _lib.dptr(w)))
    # a non-NULL handle is never dereferenced before the pointer checks fail
    fake = C.c_void_p(C.addressof(C.create_string_buffer(8)))
    _err(lib.slam_graph_chi2(fake, None, _lib.dptr(c), _lib.dptr(w)))
    # kind and parameter are checked before the handle is written
    for kind, param in ((4, 1.0), (-1, 1.0), (1, float("nan")), (2, float("inf")), (0, float("nan")),
                        (1, 0.0), (2, -1.0), (3, 0.0)):
        assert "slam_graph_set_robust" in _err(lib.slam_graph_set_robust(fake, kind, param))
    assert np.all(tot == 7.0) and np.all(c == 7.0) and np.all(w == 7.0)


def test_front_end_keywords():
    from graph_based_slam import Robot, TrajectoryEstimator
    from slamhip.graph import DeviceGraph
    p = inspect.signature(DeviceGraph.__init__).parameters
    assert list(p)[-1] == "robust" and p["robust"].default is None
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in p.items() if k != "self")
    p = inspect.signature(DeviceGraph.set_robust).parameters
    assert list(p) == ["self", "kind", "param"] and p["param"].default is None
    p = inspect.signature(DeviceGraph.chi2).parameters
    assert list(p) == ["self", "per_edge"] and p["per_edge"].default is False
    assert list(inspect.signature(DeviceGraph.edge_weights).parameters) == ["self"]
    p = inspect.signature(TrajectoryEstimator.__init__).parameters
    assert list(p) == ["self", "aPose", "solver", "device", "robust"]
    assert (p["solver"].default, p["device"].default, p["robust"].default) == ("auto", 0, None)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("solver", "device", "robust"))
    assert list(inspect.signature(TrajectoryEstimator.getEdgeWeights).parameters) == ["self"]
    p = inspect.signature(Robot.__init__).parameters
    assert list(p) == ["self", "aPose", "aDt", "aScanRng_m", "aScanAng_rad", "aLandMarks", "device",
                       "robust"]
    assert p["robust"].default is None and p["robust"].kind is inspect.Parameter.KEYWORD_ONLY
