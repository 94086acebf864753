"""The preconditioner entry points (slam_graph_set_precond, slam_graph_precond_info,
slam_graph_apply_precond) without a GPU: the exports, their
declarations, bindings and the contract in the header, the argument checks that
come before the handle is read or written, and the front ends' methods.  The
checks that need a real handle -- a bad segment and apply_precond before any
assembly leave the handle as it was -- are in test_gpu_graph_chain.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from slamhip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slam_hip.h")
P, D = C.c_void_p, C.POINTER(C.c_double)
EXPORTS = {"slam_graph_set_precond": (C.c_int, [P, C.c_int32, C.c_int32]),
           "slam_graph_precond_info": (C.c_int, [P, D]),
           "slam_graph_apply_precond": (C.c_int, [P, D, D])}


def test_exports_declared_bound_and_documented():
    text = open(HEADER).read()
    lib = _lib.load()
    for name, sig in EXPORTS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name) and _lib.SIGNATURES[name] == sig, name
    assert re.search(r"#define\s+SLAM_GRAPH_PRECOND_BLOCK_JACOBI\s+0\b", text)
    assert re.search(r"#define\s+SLAM_GRAPH_PRECOND_CHAIN\s+1\b", text)
    assert _lib.GRAPH_PRECOND == {"block_jacobi": 0, "chain": 1}
    # the contract is part of the header
    doc = text[text.index("Preconditioner of the PCG path (DESIGN 8.5"):text.index("int slam_graph_set_precond")]
    for phrase in ("S_r = D_r at a segment start, else D_r - U_{r-1}^T G_{r-1}", "G_r = Sinv_r U_r",
                   "y_r = r_r - G_{r-1}^T y_{r-1}", "z_r = Sinv_r y_r - G_r z_{r+1}",
                   "1, 2, 4, 8, 16, 32 or 64 (0 means 64", "ignored for block-Jacobi", "SLAM_ERR_ARG",
                   "before the handle changes", "next\n * linearisation", "the same bits",
                   "dense path it is accepted and has no effect", "bad pivot", "is_calc = 0",
                   "nothing has been assembled since slam_graph_set_edges", "moves no pose",
                   "off-diagonal blocks"):
        assert phrase in doc, phrase
    # slam_graph_config keeps its layout: no new field
    assert C.sizeof(_lib.GraphConfig) == 80


def _err(rc, name):
    assert rc == _lib.SLAM_ERR_ARG
    msg = _lib.load().slam_last_error().decode()
    assert name in msg, msg
    return msg


def test_argument_errors_before_the_handle_is_touched():
    lib = _lib.load()
    out = np.full(4, 7.0)
    vec = np.full(6, 7.0)
    dp = lambda a: a.ctypes.data_as(D)
    assert "NULL handle" in _err(lib.slam_graph_set_precond(None, 1, 64), "slam_graph_set_precond")
    assert "NULL" in _err(lib.slam_graph_precond_info(None, dp(out)), "slam_graph_precond_info")
    assert "NULL" in _err(lib.slam_graph_apply_precond(None, dp(vec), dp(vec)), "slam_graph_apply_precond")
    # a non-NULL handle is neither read nor written before kind and segment are
    # checked: eight bytes of a pattern that no check may touch
    buf = C.create_string_buffer(b"\x5a" * 8, 8)
    fake = C.c_void_p(C.addressof(buf))
    for kind in (-1, 2, 7):
        assert "unknown kind" in _err(lib.slam_graph_set_precond(fake, kind, 64), "slam_graph_set_precond")
    for seg in (-1, 3, 5, 6, 12, 48, 63, 65, 128, 1 << 20):
        assert "segment must be" in _err(lib.slam_graph_set_precond(fake, 1, seg), "slam_graph_set_precond")
    assert "NULL" in _err(lib.slam_graph_precond_info(fake, None), "slam_graph_precond_info")
    assert "NULL" in _err(lib.slam_graph_apply_precond(fake, None, dp(vec)), "slam_graph_apply_precond")
    assert "NULL" in _err(lib.slam_graph_apply_precond(fake, dp(vec), None), "slam_graph_apply_precond")
    assert buf.raw == b"\x5a" * 8
    # nothing assembled: the check reads the handle only (an all-zero block far
    # larger than the handle) and comes before any HIP call
    zero = C.create_string_buffer(1 << 16)
    blank = C.c_void_p(C.addressof(zero))
    assert "no system assembled" in _err(lib.slam_graph_apply_precond(blank, dp(vec), dp(vec)),
                                         "slam_graph_apply_precond")
    assert zero.raw == bytes(1 << 16)
    assert np.all(out == 7.0) and np.all(vec == 7.0)          # no output was written


def test_front_end_methods():
    """The constructors' keyword lists are pinned by test_graph_odom_capi.py and
    test_graph_robust_capi.py, so the preconditioner is chosen through methods,
    as odometry is (setOdometry)."""
    from graph_based_slam import Robot, TrajectoryEstimator
    from slamhip.graph import DeviceGraph
    p = inspect.signature(DeviceGraph.set_precond).parameters
    assert list(p) == ["self", "kind", "segment"] and p["segment"].default is None
    assert list(inspect.signature(DeviceGraph.precond_info).parameters) == ["self"]
    assert list(inspect.signature(DeviceGraph.apply_precond).parameters) == ["self", "r"]
    assert list(inspect.signature(TrajectoryEstimator.setPrecond).parameters) == ["self", "precond"]
    assert not hasattr(Robot, "setPrecond")                   # its graphs take the dense path


def test_python_argument_errors_before_the_library_call():
    from slamhip.graph import DeviceGraph
    dev = object.__new__(DeviceGraph)                         # no handle: the checks come first
    dev._h = None
    for bad in ("jacobi", "ilu", 3):
        try:
            DeviceGraph.set_precond(dev, bad)
        except ValueError as e:
            assert "precond kind" in str(e)
        else:
            raise AssertionError(bad)
    for bad in (("chain",), ("chain", 4, 4)):
        try:
            DeviceGraph.set_precond(dev, bad)
        except ValueError as e:
            assert "(kind, segment)" in str(e)
        else:
            raise AssertionError(bad)
