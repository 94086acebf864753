"""ekf_slam.EKFSLAM, the front end: the docstring example's world (a robot on
the reference's circle, a ScanSensor of 9 m range, no ids) must end with as
many landmarks as the sensor saw at p_new = 1e-4 -- checked first on the
oracle, fed the very scans the sensor produced -- and takes all three forms of
a step's observations."""
import numpy as np
import pytest

from conftest import PKG  # noqa: F401

import ekf_oracle as eo
import ekfslam_da_ref as dr

pytestmark = pytest.mark.gpu

NOISE = (0.1, np.deg2rad(3.0), np.deg2rad(3.0))          # ScanSensor's defaults


def test_docstring_world_maps_every_landmark_seen():
    from ekf_slam import EKFSLAM
    from graph_based_slam import ScanSensor
    lm = np.random.RandomState(3).uniform(-12, 12, (7, 2))
    sensor = ScanSensor(9.0, np.deg2rad(180.0), lm)
    np.random.seed(1)
    v, w, dt = 10.0 * np.deg2rad(10.0), np.deg2rad(10.0), 0.1
    pose = np.array([10.0, 0.0, np.pi / 2])
    cap, lpn = 32, float(np.log(1e-4))
    mu, P = dr.empty_state(cap)
    count, seen = 0, set()
    with EKFSLAM(cap) as a, EKFSLAM(cap) as b, EKFSLAM(cap) as c:
        for _ in range(100):
            pose = pose + np.array([v * dt * np.cos(pose[2]), v * dt * np.sin(pose[2]), w * dt])
            noisy, _ = sensor.scan(pose)
            ids = np.array([o.getLandMarkId() for o in noisy], dtype=np.int64)
            obs = np.array([[o.getDist(), o.getDir(), o.getOrient()] for o in noisy]).reshape(-1, 3)
            seen |= set(ids.tolist())
            # the oracle on the same scans
            na = 3 + 3 * count
            mu, P = mu.copy(), P.copy()
            mu[:na], P[:na, :na] = eo.ekfslam_predict(mu[:na], P[:na, :na], (v, w), dt, dr.Q_ROBOT)
            r = dr.observe(mu, P, count, cap, obs, lpn, NOISE)
            mu, P, count = r["mu"], r["P"], r["count"]
            ea, ca, (ma, pa) = a.step((v, w), noisy)
            eb, cb, (mb, pb) = b.step((v, w), (None, obs))
            ec, cc, (mc, pc) = c.step((v, w), (ids, obs))
            assert np.array_equal(a.last_assoc, r["assoc"])
            for e, cv, m, p in ((eb, cb, mb, pb), (ec, cc, mc, pc)):
                assert np.array_equal(ea, e) and np.array_equal(ca, cv)
                assert np.array_equal(ma, m) and np.array_equal(pa, p)
        assert count == len(seen) and 0 < len(seen) < len(lm)        # the oracle, a limited range
        assert a.count == count and ma.shape == (count, 3) and pa.shape == (count, 3, 3)
    # the device against the float64 oracle after 100 steps on its own state:
    # rounding differences of ~1e-15 per step, no decision apart
    assert np.abs(ea - mu[:3]).max() < 1e-9 and np.abs(ma.ravel() - mu[3:3 + 3 * count]).max() < 1e-9
    assert all(np.linalg.eigvalsh(p).min() > 0 for p in pa) and np.linalg.eigvalsh(ca).min() > 0


def test_known_ids_front_end_needs_ids():
    from ekf_slam import EKFSLAM
    with EKFSLAM(3, association=None) as s:
        with pytest.raises(ValueError, match="ids"):
            s.step((1.0, 0.1), (None, np.array([[2.0, 0.1, 0.2]])))
        pose, cov, (mean, mcov) = s.step((1.0, 0.1), (np.empty(0, int), np.empty((0, 3))))
        assert s.count == 3 and mean.shape == (3, 3) and mcov.shape == (3, 3, 3)
        assert pose[1] > 0.0 and cov[0, 0] > 1e-4            # the prediction ran
