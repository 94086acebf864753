"""fast_slam.FastSLAM, the front end: a robot on the reference's circle with a
limited-range ScanSensor, fed once with Observation objects and once with
(ids, obs) arrays."""
import numpy as np
import pytest

from conftest import PKG  # noqa: F401

pytestmark = pytest.mark.gpu


def test_frontend_takes_both_observation_forms_and_builds_a_map():
    from fast_slam import FastSLAM
    from graph_based_slam import ScanSensor
    lm = np.random.RandomState(3).uniform(-12, 12, (7, 2))
    sensor = ScanSensor(9.0, np.deg2rad(180.0), lm)
    r_dist, r_dir, r_orient = ScanSensor._R_Dist, ScanSensor._R_DirSigma, ScanSensor._R_OrientSigma
    v, w, dt = 10.0 * np.deg2rad(10.0), np.deg2rad(10.0), 0.1
    pose = np.array([10.0, 0.0, np.pi / 2])
    np.random.seed(4)
    kw = dict(noise=(r_dist, r_dir, r_orient), ess_threshold=1024, seed=1)
    observed = np.zeros(len(lm), dtype=int)
    with FastSLAM(2048, len(lm), **kw) as a, FastSLAM(2048, len(lm), **kw) as b:
        for _ in range(30):
            pose = pose + np.array([v * dt * np.cos(pose[2]), v * dt * np.sin(pose[2]), w * dt])
            noisy, _ = sensor.scan(pose)
            ids = np.array([o.getLandMarkId() for o in noisy], dtype=np.int64)
            obs = np.array([[o.getDist(), o.getDir(), o.getOrient()] for o in noisy]).reshape(-1, 3)
            observed[ids] += 1
            ea, ca, (sa, ma, pa) = a.step((v, w), noisy)
            eb, cb, (sb, mb, pb) = b.step((v, w), (ids, obs))
            assert np.array_equal(ea, eb) and np.array_equal(ca, cb)
            assert np.array_equal(ma, mb, equal_nan=True) and np.array_equal(pa, pb, equal_nan=True)
            assert np.array_equal(sa.astype(bool), observed > 0)
        assert (observed > 0).any() and not (observed > 0).all()      # a limited range
        # the pose: the particles carry 3 cm / 2 deg of process noise per step
        assert np.hypot(*(ea[:2] - pose[:2])) < 1.0
        # the map: a single observation at the sensor's range has a 0.9 m range
        # sigma and 9 m x sin(3 deg) = 0.47 m across; three sigmas of that bound
        # any landmark's estimate, however rarely it was seen
        seen = observed > 0
        assert np.isfinite(ma[seen]).all() and np.isnan(ma[~seen]).all()
        assert np.max(np.hypot(*(ma[seen] - lm[seen]).T)) < 3.0
        assert (pa[seen][:, 0] > 0).all() and (pa[seen][:, 2] > 0).all()
