"""Particle-filter ensemble, CPU side: slam_pfb_*'s argument checks return
SLAM_ERR_ARG before any HIP call (no device needed), and BatchParticleFilter's
per-filter keywords broadcast as documented (pure Python on the config array)."""
import ctypes as C

import numpy as np
import pytest

from conftest import PKG  # noqa: F401  (puts the package on sys.path)


@pytest.fixture(scope="module")
def lib():
    from slamhip import _lib
    return _lib.load()


def _create(lib, cfgs, b, n, nl, lm=None, out=True):
    from slamhip._lib import dptr
    h = C.c_void_p()
    lm = np.zeros((max(b, 1), max(nl, 1), 2)) if lm is None else lm
    rc = lib.slam_pfb_create(cfgs, b, n, nl, dptr(lm), 0, C.byref(h) if out else None)
    assert not h.value
    return rc, lib.slam_last_error().decode()


def test_create_argument_errors_without_a_device(lib):
    from slamhip._lib import SLAM_ERR_ARG
    from slamhip.pf_batch import ensemble_configs
    cfgs = ensemble_configs(3, 100)
    for b, n, nl, word in ((0, 100, 5, "n_filters"), (-2, 100, 5, "n_filters"),
                           (3, 0, 5, "n_particles"), (3, 8193, 5, "n_particles"),
                           (3, 100, 0, "n_landmarks")):
        rc, msg = _create(lib, cfgs, b, n, nl)
        assert rc == SLAM_ERR_ARG and word in msg, (b, n, nl, rc, msg)
    rc, msg = _create(lib, None, 3, 100, 5)
    assert rc == SLAM_ERR_ARG and "NULL" in msg
    rc, msg = _create(lib, cfgs, 3, 100, 5, out=False)
    assert rc == SLAM_ERR_ARG and "NULL" in msg


@pytest.mark.parametrize("field,value", [("motion", 1), ("likelihood", 1), ("dt", 0.2)])
def test_create_rejects_mixed_shared_settings(lib, field, value):
    from slamhip._lib import SLAM_ERR_ARG
    from slamhip.pf_batch import ensemble_configs
    cfgs = ensemble_configs(4, 64)
    setattr(cfgs[2], field, value)
    rc, msg = _create(lib, cfgs, 4, 64, 3)
    assert rc == SLAM_ERR_ARG and "must agree" in msg


def test_null_handles_are_argument_errors(lib):
    from slamhip._lib import SLAM_ERR_ARG, PFResult
    d = (C.c_double * 8)()
    i32 = (C.c_int32 * 2)()
    i64 = (C.c_int64 * 2)()
    res = (PFResult * 1)()
    ms, cnt = C.c_double(), C.c_int64()
    calls = [lambda: lib.slam_pfb_info(None, i32, i32, i32),
             lambda: lib.slam_pfb_set_state(None, d, d, d, d),
             lambda: lib.slam_pfb_get_state(None, d, d, d, d),
             lambda: lib.slam_pfb_get_weights_raw(None, d, d),
             lambda: lib.slam_pfb_set_resample_next(None, i32),
             lambda: lib.slam_pfb_set_ess_band(None, 1e-9),
             lambda: lib.slam_pfb_step(None, d, d, None, None, res),
             lambda: lib.slam_pfb_load_observations(None, 1, d),
             lambda: lib.slam_pfb_run(None, 0, 1, d, res),
             lambda: lib.slam_pfb_resample_indices(None, None, i64),
             lambda: lib.slam_pfb_timing(None, C.byref(ms), C.byref(cnt))]
    for k, f in enumerate(calls):
        assert f() == SLAM_ERR_ARG, k
        assert lib.slam_last_error()
    assert lib.slam_pfb_destroy(None) == 0


def test_broadcasting_of_per_filter_keywords():
    from slamhip.pf_batch import ensemble_configs
    B = 5
    r1 = np.diag([0.2, 0.4]) ** 2
    cfgs = ensemble_configs(B, 200, r=r1)
    assert all(list(c.r_cov) == list(r1.ravel()) for c in cfgs)
    cfgs = ensemble_configs(B, 200, r=0.09)                 # a scalar: that variance, every filter
    assert all(list(c.r_cov) == [0.09, 0.0, 0.0, 0.09] for c in cfgs)
    al = np.arange(B * 6, dtype=float).reshape(B, 6) / 100
    x0 = np.arange(B * 3, dtype=float).reshape(B, 3)
    cfgs = ensemble_configs(B, 200, alphas=al, x0=x0, seed=np.arange(7, 7 + B),
                            ess_threshold=np.linspace(10, 50, B), motion="velocity")
    for b, c in enumerate(cfgs):
        assert list(c.alphas) == list(al[b]) and list(c.x0) == list(x0[b])
        assert c.seed == 7 + b and c.ess_threshold == np.linspace(10, 50, B)[b]
        assert c.motion == 1 and c.dt == 0.1
    assert all(c.ess_threshold == 2.0 for c in ensemble_configs(B, 200))   # NP / 100
    for kw in (dict(alphas=np.zeros((B + 1, 6))), dict(r=np.zeros((B - 1, 2, 2))),
               dict(x0=np.zeros((B + 1, 3))), dict(seed=np.arange(B + 1)),
               dict(ess_threshold=np.ones(B + 2)), dict(q=np.zeros((2, 3, 3)))):
        with pytest.raises(ValueError):
            ensemble_configs(B, 200, **kw)
    for kw in (dict(motion=["linear"] * B), dict(dt=np.full(B, 0.1))):
        with pytest.raises(ValueError):
            ensemble_configs(B, 200, **kw)


def test_landmark_shapes_are_checked_before_the_library_call():
    from slamhip.pf_batch import BatchParticleFilter
    with pytest.raises(ValueError):
        BatchParticleFilter(3, 100, np.zeros((4, 5, 2)))
    with pytest.raises(ValueError):
        BatchParticleFilter(3, 100, np.zeros((5, 3)))
