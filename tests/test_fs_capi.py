"""FastSLAM C-ABI, CPU side: slam_fs_*'s argument checks return SLAM_ERR_ARG
before any HIP call (no device needed)."""
import ctypes as C

import numpy as np
import pytest

from conftest import PKG  # noqa: F401  (puts the package on sys.path)


@pytest.fixture(scope="module")
def lib():
    from slamhip import _lib
    return _lib.load()


def _check(lib, nl, ids, obs):
    from slamhip._lib import _I64, dptr
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, 3)
    rc = lib.slam_fs_check_observations(nl, ids.size, ids.ctypes.data_as(_I64), dptr(obs))
    return rc, lib.slam_last_error().decode()


GOOD = [[2.0, 0.1, 0.2], [3.0, -0.4, 0.2], [1.5, 3.0, 0.2]]


def test_observation_rules_without_a_device(lib):
    from slamhip._lib import SLAM_ERR_ARG, SLAM_OK
    assert _check(lib, 5, [0, 4, 2], GOOD)[0] == SLAM_OK
    assert _check(lib, 5, [], np.zeros((0, 3)))[0] == SLAM_OK            # an empty step
    rc, msg = _check(lib, 2, [0, 1, 1], GOOD)                            # k > NL
    assert rc == SLAM_ERR_ARG and "k" in msg
    rc, msg = _check(lib, 5, [0, 4, 0], GOOD)
    assert rc == SLAM_ERR_ARG and "duplicate" in msg
    for bad in (5, -1):
        rc, msg = _check(lib, 5, [0, bad, 2], GOOD)
        assert rc == SLAM_ERR_ARG and "out of range" in msg
    for d in (0.0, -1.0):
        rc, msg = _check(lib, 5, [0, 4, 2], [[2.0, 0.1, 0.2], [d, 0.0, 0.0], [1.5, 3.0, 0.2]])
        assert rc == SLAM_ERR_ARG and "d <= 0" in msg
    for col, v in ((0, np.nan), (1, np.inf), (2, -np.inf)):
        o = np.array(GOOD)
        o[1, col] = v
        rc, msg = _check(lib, 5, [0, 4, 2], o)
        assert rc == SLAM_ERR_ARG and "non-finite" in msg
    assert lib.slam_fs_check_observations(5, -1, None, None) == SLAM_ERR_ARG
    assert lib.slam_fs_check_observations(5, 2, None, None) == SLAM_ERR_ARG
    assert lib.slam_fs_check_observations(0, 0, None, None) == SLAM_ERR_ARG


def test_create_argument_errors_without_a_device(lib):
    from slamhip._lib import SLAM_ERR_ARG, FSConfig
    from slamhip.pf import make_config

    def cfg(**kw):
        c = FSConfig()
        c.pf = make_config(100)
        c.r_dist, c.r_dir, c.r_orient, c.use_orient = 0.1, 0.05, 0.05, 1
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def create(c, n, nl, out=True):
        h = C.c_void_p()
        rc = lib.slam_fs_create(None if c is None else C.byref(c), n, nl, 0,
                                C.byref(h) if out else None)
        assert not h.value
        return rc, lib.slam_last_error().decode()

    for n, nl, word in ((0, 3, "n_particles"), ((1 << 24) + 1, 3, "n_particles"),
                        (100, 0, "n_landmarks"), (100, -1, "n_landmarks")):
        rc, msg = create(cfg(), n, nl)
        assert rc == SLAM_ERR_ARG and word in msg, (n, nl, rc, msg)
    assert create(None, 100, 3)[0] == SLAM_ERR_ARG
    assert create(cfg(), 100, 3, out=False)[0] == SLAM_ERR_ARG
    rc, msg = create(cfg(r_dist=0.0), 100, 3)
    assert rc == SLAM_ERR_ARG and "r_dist" in msg
    bad = cfg()
    bad.pf.motion = 7
    rc, msg = create(bad, 100, 3)
    assert rc == SLAM_ERR_ARG and "motion" in msg


def test_null_handles_are_argument_errors(lib):
    from slamhip._lib import SLAM_ERR_ARG, PFResult
    d = (C.c_double * 8)()
    i32 = (C.c_int32 * 2)()
    i64 = (C.c_int64 * 2)()
    n64 = C.c_int64()
    res = (PFResult * 1)()
    calls = [lambda: lib.slam_fs_info(None, C.byref(n64), i32, i32),
             lambda: lib.slam_fs_set_state(None, d, d, d, d),
             lambda: lib.slam_fs_get_state(None, d, d, d, d),
             lambda: lib.slam_fs_set_resample_next(None, 1),
             lambda: lib.slam_fs_set_maps(None, i32, d, d),
             lambda: lib.slam_fs_get_maps(None, i32, d, d),
             lambda: lib.slam_fs_get_map(None, 0, i32, d, d),
             lambda: lib.slam_fs_step(None, d, 0, i64, d, None, 0.5, res),
             lambda: lib.slam_fs_resample(None, 0.5, 1, i32),
             lambda: lib.slam_fs_predict(None, d, None),
             lambda: lib.slam_fs_update(None, 0, i64, d, res),
             lambda: lib.slam_fs_load_observations(None, 1, i32, i64, d),
             lambda: lib.slam_fs_run(None, 0, 1, d, res),
             lambda: lib.slam_fs_timing(None, d)]
    for k, f in enumerate(calls):
        assert f() == SLAM_ERR_ARG, k
        assert lib.slam_last_error()
    assert lib.slam_fs_destroy(None) == 0


def test_config_struct_matches_the_header():
    from slamhip._lib import FSConfig, PFConfig
    assert C.sizeof(FSConfig) == C.sizeof(PFConfig) + 3 * 8 + 2 * 4
    assert FSConfig.r_dist.offset == C.sizeof(PFConfig)
