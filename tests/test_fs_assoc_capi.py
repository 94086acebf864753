"""Associating FastSLAM handles, C-ABI, CPU side: slam_fs_create_assoc's
argument checks return SLAM_ERR_ARG before any HIP call (no device needed),
the new accessors refuse NULL handles, and the ctypes struct matches the
header."""
import ctypes as C

import numpy as np
import pytest

from conftest import PKG  # noqa: F401  (puts the package on sys.path)


@pytest.fixture(scope="module")
def lib():
    from slamhip import _lib
    return _lib.load()


def _cfg(**kw):
    from slamhip._lib import FSConfig
    from slamhip.pf import make_config
    c = FSConfig()
    c.pf = make_config(100)
    c.r_dist, c.r_dir, c.r_orient, c.use_orient = 0.1, 0.05, 0.05, 1
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _acfg(log_p_new=np.log(0.1), record=1):
    from slamhip._lib import FSAssocConfig
    return FSAssocConfig(float(log_p_new), int(record), 0)


def test_create_assoc_argument_errors_without_a_device(lib):
    from slamhip._lib import SLAM_ERR_ARG

    def create(c, a, n, cap, out=True):
        h = C.c_void_p()
        rc = lib.slam_fs_create_assoc(None if c is None else C.byref(c),
                                      None if a is None else C.byref(a), n, cap, 0,
                                      C.byref(h) if out else None)
        assert not h.value
        return rc, lib.slam_last_error().decode()

    assert create(None, _acfg(), 100, 8)[0] == SLAM_ERR_ARG
    assert create(_cfg(), None, 100, 8)[0] == SLAM_ERR_ARG
    assert create(_cfg(), _acfg(), 100, 8, out=False)[0] == SLAM_ERR_ARG
    for cap in (0, -3):
        rc, msg = create(_cfg(), _acfg(), 100, cap)
        assert rc == SLAM_ERR_ARG and "max_landmarks" in msg, (cap, rc, msg)
    for v in (np.nan, np.inf, -np.inf):
        rc, msg = create(_cfg(), _acfg(log_p_new=v), 100, 8)
        assert rc == SLAM_ERR_ARG and "log_p_new" in msg, (v, rc, msg)
    for n in (0, -1, (1 << 24) + 1):
        rc, msg = create(_cfg(), _acfg(), n, 8)
        assert rc == SLAM_ERR_ARG and "n_particles" in msg, (n, rc, msg)
    # the shared rules of slam_fs_create still hold
    rc, msg = create(_cfg(r_dist=0.0), _acfg(), 100, 8)
    assert rc == SLAM_ERR_ARG and "r_dist" in msg


def test_null_handles_are_argument_errors(lib):
    from slamhip._lib import SLAM_ERR_ARG
    i32 = (C.c_int32 * 4)()
    for k, f in enumerate((lambda: lib.slam_fs_set_counts(None, i32),
                           lambda: lib.slam_fs_get_counts(None, i32),
                           lambda: lib.slam_fs_get_assoc(None, i32))):
        assert f() == SLAM_ERR_ARG, k
        assert lib.slam_last_error()


def test_config_struct_matches_the_header():
    from slamhip import _lib
    assert C.sizeof(_lib.FSAssocConfig) == 16
    assert _lib.FSAssocConfig.log_p_new.offset == 0 and _lib.FSAssocConfig.record.offset == 8
    assert _lib.FS_ASSOC_MAX_OBS >= 4096
    for name in ("slam_fs_create_assoc", "slam_fs_set_counts", "slam_fs_get_counts",
                 "slam_fs_get_assoc"):
        assert name in _lib.SIGNATURES
