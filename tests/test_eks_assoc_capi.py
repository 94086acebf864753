"""Associating EKF-SLAM handles, C-ABI, CPU side: slam_ekfslam_create_assoc's
argument checks and slam_ekfslam_check_observations return SLAM_ERR_ARG before
any HIP call (no device needed), the new entry points refuse NULL handles, and
the ctypes structs match the header."""
import ctypes as C

import numpy as np
import pytest

from conftest import PKG  # noqa: F401  (puts the package on sys.path)


@pytest.fixture(scope="module")
def lib():
    from slamhip import _lib
    return _lib.load()


def _cfg():
    from slamhip._lib import EKFSLAMConfig
    c = EKFSLAMConfig()
    c.dt = 0.1
    c.q_robot[:] = [float(v) for v in np.diag([0.01, 0.01, 1e-6]).ravel()]
    c.r_dist, c.r_dir, c.r_orient = 0.05, 0.03, 0.03
    return c


def _acfg(log_p_new=np.log(1e-4), record=1):
    from slamhip._lib import EKFSLAMAssocConfig
    return EKFSLAMAssocConfig(float(log_p_new), int(record), 0)


def test_create_assoc_argument_errors_without_a_device(lib):
    from slamhip._lib import SLAM_ERR_ARG

    def create(c, a, cap, out=True):
        h = C.c_void_p()
        rc = lib.slam_ekfslam_create_assoc(None if c is None else C.byref(c),
                                           None if a is None else C.byref(a), cap, 0,
                                           C.byref(h) if out else None)
        assert not h.value
        return rc, lib.slam_last_error().decode()

    assert create(None, _acfg(), 8)[0] == SLAM_ERR_ARG
    assert create(_cfg(), None, 8)[0] == SLAM_ERR_ARG
    assert create(_cfg(), _acfg(), 8, out=False)[0] == SLAM_ERR_ARG
    for cap in (0, -3):
        rc, msg = create(_cfg(), _acfg(), cap)
        assert rc == SLAM_ERR_ARG and "capacity" in msg, (cap, rc, msg)
    for v in (np.nan, np.inf, -np.inf):
        rc, msg = create(_cfg(), _acfg(log_p_new=v), 8)
        assert rc == SLAM_ERR_ARG and "log_p_new" in msg, (v, rc, msg)


def test_check_observations(lib):
    from slamhip._lib import SLAM_ERR_ARG, SLAM_OK, dptr
    good = np.tile([2.0, 0.1, -0.2], (41, 1))
    check = lib.slam_ekfslam_check_observations
    assert check(0, None) == SLAM_OK
    assert check(40, dptr(good)) == SLAM_OK
    assert check(41, dptr(good)) == SLAM_ERR_ARG and b"k <= 40" in lib.slam_last_error()
    assert check(-1, dptr(good)) == SLAM_ERR_ARG
    assert check(3, None) == SLAM_ERR_ARG
    for col, v in ((0, np.nan), (1, np.nan), (2, np.inf), (1, -np.inf)):
        bad = good[:5].copy()
        bad[3, col] = v
        assert check(5, dptr(bad)) == SLAM_ERR_ARG and b"finite" in lib.slam_last_error(), (col, v)
    for v in (0.0, -1.0):
        bad = good[:5].copy()
        bad[4, 0] = v
        assert check(5, dptr(bad)) == SLAM_ERR_ARG and b"positive" in lib.slam_last_error(), v


def test_null_handles_are_argument_errors(lib):
    from slamhip._lib import SLAM_ERR_ARG, EKFSLAMAssocInfo, dptr
    i32 = (C.c_int32 * 4)()
    obs = np.array([[2.0, 0.1, 0.2]])
    out = np.zeros(4)
    ctl = np.array([1.0, 0.1])
    info = EKFSLAMAssocInfo()
    for k, f in enumerate((lambda: lib.slam_ekfslam_observe(None, 1, dptr(obs), i32),
                           lambda: lib.slam_ekfslam_step_assoc(None, dptr(ctl), 1, dptr(obs), i32),
                           lambda: lib.slam_ekfslam_get_count(None, i32),
                           lambda: lib.slam_ekfslam_set_count(None, 0),
                           lambda: lib.slam_ekfslam_get_scores(None, dptr(out)),
                           lambda: lib.slam_ekfslam_assoc_info(None, C.byref(info)),
                           lambda: lib.slam_ekfslam_assoc_timing(None, dptr(out)))):
        assert f() == SLAM_ERR_ARG, k
        assert lib.slam_last_error()


def test_structs_match_the_header():
    from slamhip import _lib
    a = _lib.EKFSLAMAssocConfig
    assert C.sizeof(a) == 16 and a.log_p_new.offset == 0 and a.record.offset == 8 and a.pad.offset == 12
    i = _lib.EKFSLAMAssocInfo
    assert C.sizeof(i) == 40
    assert [getattr(i, f).offset for f, _ in i._fields_] == [0, 8, 16, 20, 24, 28, 32, 36]
    assert _lib.EKS_ASSOC_MAX_OBS == 40
    for name in ("slam_ekfslam_create_assoc", "slam_ekfslam_observe", "slam_ekfslam_step_assoc",
                 "slam_ekfslam_get_count", "slam_ekfslam_set_count", "slam_ekfslam_get_scores",
                 "slam_ekfslam_assoc_info", "slam_ekfslam_assoc_timing",
                 "slam_ekfslam_check_observations"):
        assert name in _lib.SIGNATURES
