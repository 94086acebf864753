"""EKF-SLAM on the MI355X kernels (libslam_hip.so): one Gaussian over the robot
pose and every landmark (x, y, phi), its covariance in HBM -- an extension, the
reference has no EKF-SLAM.  The counterpart of fast_slam.FastSLAM: both take
the same scans and can be compared.

``EKFSLAM(capacity)`` starts with an empty map.  ``step(control,
observations)`` takes what a limited-range sensor saw this step -- ``(None,
obs)`` with ``obs`` rows (range, bearing, orientation), ``(ids, obs)``, or the
list of ``Observation`` objects that ``ScanSensor.scan`` returns -- and returns
the pose, its 3 x 3 covariance and the map ``(mean [count][3], cov
[count][3][3])``.  A real sensor does not know which landmark it saw: ids are
dropped, every observation is matched to the likeliest landmark held (each
landmark at most once per scan) or, below the likelihood ``p_new``, starts a new
one, and the update walks only the rows of the landmarks held so far.

A headless example: a robot on the reference's circle with a scan sensor of
9 m range::

    import numpy as np
    from ekf_slam import EKFSLAM
    from graph_based_slam import ScanSensor

    landmarks = np.random.RandomState(3).uniform(-12, 12, (7, 2))
    sensor = ScanSensor(9.0, np.deg2rad(180.0), landmarks)
    np.random.seed(1)
    slam = EKFSLAM(32)
    pose = np.array([10.0, 0.0, np.pi / 2])
    v, w, dt = 10.0 * np.deg2rad(10.0), np.deg2rad(10.0), 0.1
    for _ in range(100):
        pose = pose + np.array([v * dt * np.cos(pose[2]), v * dt * np.sin(pose[2]), w * dt])
        noisy, _ = sensor.scan(pose)
        est, cov, (mean, mcov) = slam.step((v, w), noisy)
    print(est, slam.count, mean)
    slam.close()

``EKFSLAM(n_landmarks, association=None)`` is EKF-SLAM with known ids (a
simulator's): every landmark must then be given before the first step
(``dev.set_state`` or ``dev.init_diag``), and ``step`` needs the ids.
"""
from __future__ import annotations

import numpy as np

from fast_slam import _split
from slamhip.ekf import DeviceEKFSLAM

X0 = (10.0, 0.0, np.pi / 2)                    # the reference's start pose
P0 = (1e-4, 1e-4, 1e-6)


class EKFSLAM:
    """Keyword arguments are DeviceEKFSLAM's (dt, q_robot, noise=(r_dist, r_dir,
    r_orient), motion, alphas, device, p_new, record_assoc, prune); the
    measurement noise defaults to ScanSensor's (10 %, 3 deg, 3 deg).  ``x0`` /
    ``p0``: the start pose and the diagonal of its covariance.
    ``prune=dict(view_range=...)`` (FastSLAM's keywords) removes landmarks that
    stay unmatched in view: ``count`` and ``map()`` then shrink as well."""

    def __init__(self, capacity, *, association="ml", x0=X0, p0=P0, **kw):
        kw.setdefault("noise", (0.1, np.deg2rad(3.0), np.deg2rad(3.0)))
        self.dev = DeviceEKFSLAM(capacity, association=association, **kw)
        mu, diag = np.zeros(self.dev.n), np.zeros(self.dev.n)
        mu[:3], diag[:3] = x0, p0
        self.dev.init_diag(mu, diag)
        self.last_assoc = None

    @property
    def count(self):
        """Landmarks held (the capacity, with known ids)."""
        return self.dev.count if self.dev.association else self.dev.n_lm

    def step(self, control, observations):
        """One step: returns (pose (3,), cov (3, 3), (mean [count][3],
        cov [count][3][3]))."""
        ids, obs = _split(observations)
        if self.dev.association:
            self.last_assoc = self.dev.step(control, None, obs)
        elif ids is None:
            raise ValueError("EKFSLAM(association=None) needs the observations' ids")
        elif len(ids):
            self.dev.step(control, ids, obs)
        else:
            self.dev.predict(control)
        pose, cov = self.dev.pose()
        return pose, cov, self.map()

    def map(self):
        """(mean [count][3], cov [count][3][3]) of the landmarks held."""
        if self.dev.association:
            return self.dev.landmarks()
        mu, P = self.dev.get_state()
        n_lm = self.dev.n_lm
        blocks = np.array([P[3 + 3 * j:6 + 3 * j, 3 + 3 * j:6 + 3 * j] for j in range(n_lm)])
        return mu[3:].reshape(n_lm, 3), blocks.reshape(n_lm, 3, 3)

    def close(self):
        self.dev.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
