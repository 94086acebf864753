"""FastSLAM 1.0 with known data association on the MI355X kernels
(libslam_hip.so): the particle-filter form of SLAM, an extension -- the
reference's particle filter (particle_filter.py) localises against a known map.

``FastSLAM(n_particles, n_landmarks)`` keeps, per particle, a pose and one 2-D
EKF per landmark on the GPU (slamhip.fastslam.DeviceFastSLAM).
``step(control, observations)`` takes what a limited-range sensor saw this
step -- either ``(ids, obs)`` with ``obs`` rows (range, bearing, orientation),
or the list of ``Observation`` objects that ``ScanSensor.scan`` returns -- and
returns the pose estimate, the particle covariance and the best particle's map.

A headless example: a robot on the reference's circle (particle_filter.py:46-48)
with a scan sensor of 9 m range::

    import numpy as np
    from fast_slam import FastSLAM
    from graph_based_slam import ScanSensor

    landmarks = np.random.RandomState(3).uniform(-12, 12, (7, 2))
    sensor = ScanSensor(9.0, np.deg2rad(180.0), landmarks)
    slam = FastSLAM(4096, len(landmarks), ess_threshold=2048, seed=1)
    pose = np.array([10.0, 0.0, np.pi / 2])
    v, w, dt = 10.0 * np.deg2rad(10.0), np.deg2rad(10.0), 0.1
    for _ in range(100):
        pose = pose + np.array([v * dt * np.cos(pose[2]), v * dt * np.sin(pose[2]), w * dt])
        noisy, _ = sensor.scan(pose)
        est, cov, (seen, mean, mcov) = slam.step((v, w), noisy)
    print(est, mean[seen.astype(bool)])
    slam.close()

A real range / bearing sensor does not know which landmark it saw.
``FastSLAM(n_particles, capacity, association="ml")`` drops the ids: every
particle matches an observation to the likeliest landmark of its own map, or
starts a new one (``p_new``), and ``best_map()`` is the heaviest particle's
``(seen, mean, cov)`` with ``seen[j] = j < count``.  ``step`` then also accepts
``(None, obs)``.

Such a filter also starts landmarks that are not there (a noisy sighting that
matches nothing), and by itself never takes one away.  ``prune=dict(
view_range=7.2)`` adds the existence counter of published FastSLAM: a landmark
gains evidence when it is matched, loses it when it lies in view and the scan
did not contain it, and leaves the map below a threshold (``init``, ``hit``,
``miss``, ``ev_max``, ``remove_below``, ``view_angle``: DeviceFastSLAM.
set_pruning).  Give a view range somewhat inside the sensor's -- 7.2 m for the
9 m sensor above -- so that a landmark at the edge of the range, which the
sensor may or may not return, is not counted as missed::

    slam = FastSLAM(4096, 32, association="ml", p_new=0.1,
                    prune=dict(view_range=7.2), ess_threshold=2048, seed=1)
"""
from __future__ import annotations

import numpy as np

from slamhip.fastslam import DeviceFastSLAM


def _split(observations):
    """(ids, obs) from either form of a step's observations."""
    if isinstance(observations, tuple) and len(observations) == 2 and \
            not hasattr(observations[0], "getLandMarkId"):
        ids, obs = observations
        obs = np.asarray(obs, dtype=np.float64).reshape(-1, 3)
        return (None if ids is None else np.asarray(ids, dtype=np.int64).reshape(-1)), obs
    obs_list = list(observations)
    ids = np.array([o.getLandMarkId() for o in obs_list], dtype=np.int64)
    obs = np.array([[o.getDist(), o.getDir(), o.getOrient()] for o in obs_list],
                   dtype=np.float64).reshape(-1, 3)
    return ids, obs


class FastSLAM:
    """Keyword arguments are DeviceFastSLAM's (dt, q, alphas, x0, motion,
    noise=(r_dist, r_dir, r_orient), use_orient, ess_threshold, seed, device);
    the measurement noise defaults to ScanSensor's (10 %, 3 deg, 3 deg).
    ``association="ml"``: ``n_landmarks`` is the capacity of a particle's map and
    the observations' ids are dropped (also ``p_new``, ``record_assoc``).
    ``proposal="measurement"`` (FastSLAM 2.0; known association, linear
    motion): every particle filters its pose through the step's scan and draws
    it from the resulting N(mu, Sigma).  ``step``'s ``noise`` then means three
    standard normals per particle ([NP][3], pose = mu + chol(Sigma) noise), not
    the Q-shaped motion noise of the default proposal; ``record_proposal``
    keeps mu, Sigma and the log weights for ``dev.last_proposal()``.
    ``association="ml_marginal"`` with ``proposal="measurement"``: FastSLAM 2.0
    from scans without ids -- the association runs inside the proposal, its
    score marginalising the pose; ``n_landmarks`` is the capacity.
    ``prune=dict(view_range=..., ...)`` (associating kinds only): landmark
    evidence and the removal of unsupported landmarks; ``best_map()`` is the
    compacted map."""

    def __init__(self, n_particles, n_landmarks, **kw):
        self.dev = DeviceFastSLAM(n_particles, n_landmarks, **kw)
        self.last = None

    def step(self, control, observations, noise=None, u_resample=float("nan")):
        """One step: returns (x_est (3,), cov (3, 3), (seen, mean [NL][2],
        cov [NL][3])) -- the heaviest particle's pose and map, and the
        weighted particle covariance.  The motion noise and the resampling
        offset come from the device RNG unless given (as slam_pf_step)."""
        ids, obs = _split(observations)
        if self.dev.association in ("ml", "ml_marginal"):
            ids = None
        self.last = self.dev.step(control, ids, obs, noise, u_resample)
        return self.last["x_est"], self.last["cov"], self.dev.best_map()

    def best_map(self):
        """The heaviest particle's (seen, mean [NL][2], cov [NL][3])."""
        return self.dev.best_map()

    def close(self):
        self.dev.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
