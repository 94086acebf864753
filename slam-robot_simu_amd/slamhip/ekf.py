"""Device EKF filters: handles on libslam_hip's slam_ekf_* (batched 3-state
localisation, extended_kalman_filter.py) and slam_ekfslam_* (EKF-SLAM,
BASELINE config 4) entry points."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import EKFConfig, EKFSLAMConfig, check, dptr
from .fastslam import prune_config


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


def reference_ekf_config(period_ms=100):
    """The constants of ExtendedKalmanFilter.__init__ (extended_kalman_filter.py:29-84)."""
    dt = period_ms / 1000
    omega = np.deg2rad(10.0)
    return dict(dt=dt, vel=10.0 * omega, omega=omega,
                q=np.diag([0.1, 0.1, np.deg2rad(0.1)]) ** 2,
                r=np.diag([1.0, 1.0]) ** 2,
                x0=np.array([10.0, 0.0, np.deg2rad(90.0)]),
                p0=np.diag([0.01, 0.01, np.deg2rad(30.0)]) ** 2)


_MOTIONS = {"linear": 0, "velocity": 1}
DEFAULT_ALPHAS = (0.1, 0.1, 0.1, 0.1, 0.1, 0.1)     # graph_based_slam.py:605 MotionModel(2.0, 0.1 x 6)


class DeviceEKF:
    """``batch`` independent 3-state EKFs on one GPU (batch=1: the reference's filter).

    ``motion="linear"``: the reference's prediction (extended_kalman_filter.py
    :160-194, Q).  ``motion="velocity"``: the prediction driven by
    motion_model.py (north_star) -- f = MotionModel.moveWithoutNoise, its
    Jacobian, and the process noise of moveWithNoise from ``alphas`` (a1..a6)."""

    def __init__(self, batch=1, *, device=0, motion="linear", alphas=DEFAULT_ALPHAS, **params):
        p = reference_ekf_config()
        p.update(params)
        cfg = EKFConfig()
        cfg.motion = _MOTIONS[motion]
        cfg.alphas[:] = [float(a) for a in alphas]
        self.motion = motion
        cfg.dt, cfg.vel, cfg.omega = float(p["dt"]), float(p["vel"]), float(p["omega"])
        cfg.q[:] = [float(v) for v in np.asarray(p["q"], float).ravel()]
        cfg.r[:] = [float(v) for v in np.asarray(p["r"], float).ravel()]
        cfg.x0[:] = [float(v) for v in np.asarray(p["x0"], float).ravel()]
        cfg.p0[:] = [float(v) for v in np.asarray(p["p0"], float).ravel()]
        self.batch = int(batch)
        self.params = p
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.slam_ekf_create(C.byref(cfg), self.batch, int(device), C.byref(h)),
              "slam_ekf_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.slam_ekf_destroy(self._h)
            self._h = None

    __del__ = close

    def set_state(self, x=None, P=None):
        x = None if x is None else _f64(x, (self.batch, 3))
        P = None if P is None else _f64(P, (self.batch, 9))
        check(self._lib.slam_ekf_set_state(self._h, dptr(x), dptr(P)), "slam_ekf_set_state")

    def get_state(self):
        x = np.empty((self.batch, 3))
        P = np.empty((self.batch, 3, 3))
        check(self._lib.slam_ekf_get_state(self._h, dptr(x), dptr(P)), "slam_ekf_get_state")
        return x, P

    def step(self, z, control=None):
        """One filter step; z: (batch, 2) world positions.  Returns (x_hat_m, x_hat, P)."""
        z = _f64(z, (self.batch, 2))
        ctl = None if control is None else _f64(control, (2,))
        xm = np.empty((self.batch, 3))
        xh = np.empty((self.batch, 3))
        P = np.empty((self.batch, 3, 3))
        check(self._lib.slam_ekf_step(self._h, dptr(ctl), dptr(z), dptr(xm), dptr(xh), dptr(P)),
              "slam_ekf_step")
        return xm, xh, P

    def run(self, z_all, control=None):
        """len(z_all) steps in one launch; z_all: (steps, batch, 2).  Returns x_hat (steps, batch, 3)."""
        z_all = _f64(z_all)
        steps = z_all.shape[0]
        z_all = z_all.reshape(steps, self.batch, 2)
        ctl = None if control is None else _f64(control, (2,))
        out = np.empty((steps, self.batch, 3))
        check(self._lib.slam_ekf_run(self._h, steps, dptr(ctl), dptr(z_all), dptr(out)),
              "slam_ekf_run")
        return out

    def run_device(self, n_steps, z_dev_ptr, xh_dev_ptr=None, control=None):
        """n_steps steps with observations already in device memory (pointer to
        n_steps x batch x 2 fp64); asynchronous (see synchronize)."""
        ctl = None if control is None else _f64(control, (2,))
        check(self._lib.slam_ekf_run_device(self._h, int(n_steps), dptr(ctl), C.c_void_p(z_dev_ptr),
                                            C.c_void_p(xh_dev_ptr) if xh_dev_ptr else None),
              "slam_ekf_run_device")

    def load_observations(self, z_all):
        z_all = _f64(z_all)
        steps = z_all.shape[0]
        check(self._lib.slam_ekf_load_observations(self._h, steps, dptr(z_all.reshape(steps, self.batch, 2))),
              "slam_ekf_load_observations")
        self.loaded_steps = steps

    def run_loaded(self, n_steps, control=None, keep_history=True):
        """Asynchronous: n_steps filter steps from the loaded observations."""
        ctl = None if control is None else _f64(control, (2,))
        check(self._lib.slam_ekf_run_loaded(self._h, int(n_steps), dptr(ctl), int(bool(keep_history))),
              "slam_ekf_run_loaded")

    def synchronize(self):
        check(self._lib.slam_ekf_synchronize(self._h), "slam_ekf_synchronize")


class DeviceEKFSLAM:
    """EKF-SLAM over ``n_landmarks`` landmarks (x, y, phi); covariance in HBM.

    ``association="ml"``: ``n_landmarks`` is the capacity of a map that starts
    empty.  ``observe(obs)`` / ``step(control, None, obs)`` take (range,
    bearing, orientation) rows without ids: each is matched to the likeliest
    landmark held (each landmark at most once per call) or, below ``p_new``,
    starts a new one; the update then walks the ``3 + 3 count`` active rows
    only.  ``record_assoc`` keeps the scores for ``last_scores()``.

    ``prune``: None, or ``set_pruning``'s keywords as a dict (DeviceFastSLAM's:
    both estimators take the same ones) -- every landmark then carries an
    evidence value, gains ``hit`` when matched, loses ``miss`` when it lies in
    view of the posterior pose unmatched, and is removed from ``mu`` and ``P``
    below ``remove_below``; the survivors move down in place.  ``remove(slots)``
    takes landmarks away by hand."""

    def __init__(self, n_landmarks, *, dt=0.1, q_robot=None, noise=(0.05, np.deg2rad(2.0),
                                                                         np.deg2rad(2.0)), device=0,
                 motion="linear", alphas=DEFAULT_ALPHAS, association=None, p_new=1e-4,
                 record_assoc=False, prune=None):
        if association not in (None, "ml"):
            raise ValueError(f"association must be None or 'ml', not {association!r}")
        if prune is not None and association is None:
            raise ValueError("prune needs association='ml'")
        self.association = association
        cfg = EKFSLAMConfig()
        cfg.dt = float(dt)
        cfg.motion = _MOTIONS[motion]
        cfg.alphas[:] = [float(a) for a in alphas]
        self.motion = motion
        q = np.diag([0.1, 0.1, np.deg2rad(0.1)]) ** 2 if q_robot is None else np.asarray(q_robot)
        cfg.q_robot[:] = [float(v) for v in q.ravel()]
        cfg.r_dist, cfg.r_dir, cfg.r_orient = (float(v) for v in noise)
        self.n_lm = int(n_landmarks)
        self.n = 3 + 3 * self.n_lm
        self._lib = _lib.load()
        h = C.c_void_p()
        if association is None:
            check(self._lib.slam_ekfslam_create(C.byref(cfg), self.n_lm, int(device), C.byref(h)),
                  "slam_ekfslam_create")
        else:
            acfg = _lib.EKFSLAMAssocConfig(float(np.log(p_new)), int(bool(record_assoc)), 0)
            check(self._lib.slam_ekfslam_create_assoc(C.byref(cfg), C.byref(acfg), self.n_lm,
                                                      int(device), C.byref(h)),
                  "slam_ekfslam_create_assoc")
            self._assoc = np.empty(0, dtype=np.int32)
        self._h = h
        self.prune = None
        if prune is not None:
            try:
                self.set_pruning(**prune)
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "_h", None):
            self._lib.slam_ekfslam_destroy(self._h)
            self._h = None

    __del__ = close

    def set_state(self, mu, P=None):
        mu = _f64(mu, (self.n,))
        P = None if P is None else _f64(P, (self.n, self.n))
        check(self._lib.slam_ekfslam_set_state(self._h, dptr(mu), dptr(P)), "slam_ekfslam_set_state")

    def init_diag(self, mu, p_diag):
        check(self._lib.slam_ekfslam_init_diag(self._h, dptr(_f64(mu, (self.n,))),
                                               dptr(_f64(p_diag, (self.n,)))),
              "slam_ekfslam_init_diag")

    def get_state(self, with_cov=True):
        mu = np.empty(self.n)
        P = np.empty((self.n, self.n)) if with_cov else None
        check(self._lib.slam_ekfslam_get_state(self._h, dptr(mu), dptr(P)), "slam_ekfslam_get_state")
        return (mu, P) if with_cov else mu

    def get_rows(self, rows):
        """Rows of the symmetric covariance (k x n) without copying all of P."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).ravel()
        out = np.empty((rows.size, self.n))
        check(self._lib.slam_ekfslam_get_rows(self._h, int(rows.size),
                                              rows.ctypes.data_as(C.POINTER(C.c_int64)), dptr(out)),
              "slam_ekfslam_get_rows")
        return out

    def predict(self, control):
        check(self._lib.slam_ekfslam_predict(self._h, dptr(_f64(control, (2,)))),
              "slam_ekfslam_predict")

    def update(self, ids, obs):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        obs = _f64(obs, (ids.size, 3))
        check(self._lib.slam_ekfslam_update(self._h, int(ids.size),
                                            ids.ctypes.data_as(C.POINTER(C.c_int64)), dptr(obs)),
              "slam_ekfslam_update")

    def step(self, control, ids, obs):
        """Predict and update.  ``ids=None`` (associating handle): the
        observations carry no identity; returns the association."""
        if ids is None:
            obs = _f64(obs).reshape(-1, 3)
            self._assoc = np.empty(obs.shape[0], dtype=np.int32)
            check(self._lib.slam_ekfslam_step_assoc(
                self._h, dptr(_f64(control, (2,))), int(obs.shape[0]), dptr(obs),
                self._assoc.ctypes.data_as(C.POINTER(C.c_int32))), "slam_ekfslam_step_assoc")
            return self._assoc.copy()
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        obs = _f64(obs, (ids.size, 3))
        check(self._lib.slam_ekfslam_step(self._h, dptr(_f64(control, (2,))), int(ids.size),
                                          ids.ctypes.data_as(C.POINTER(C.c_int64)), dptr(obs)),
              "slam_ekfslam_step")

    def timing(self):
        out = np.zeros(5)
        check(self._lib.slam_ekfslam_timing(self._h, dptr(out)), "slam_ekfslam_timing")
        return dict(gather_ms=out[0], inverse_ms=out[1], gain_ms=out[2], rank_update_ms=out[3])

    def info(self):
        """Sizes and resident grids of the handle, and of the last update its
        operand width ``M`` and the kernels it launched: ``rank`` in
        frag2x4 | frag2x2 | frag2x4_pf | pipe | lds, ``apply`` in mfma | lds
        (both None before the first update)."""
        s = _lib.EKFSLAMInfo()
        check(self._lib.slam_ekfslam_info(self._h, C.byref(s)), "slam_ekfslam_info")
        return dict(n=s.n, ld=s.ld, n_pad=s.n_pad, n_tiles=s.n_tiles, frag_grid=s.frag_grid,
                    pipe_grid=s.pipe_grid, M=s.last_m, rank=_lib.EKS_RANK[s.last_rank],
                    apply=_lib.EKS_APPLY[s.last_apply])

    # ------------------------------------------------ association="ml" only
    def observe(self, obs):
        """Associate, update and initialise from the current (predicted) state.
        Returns assoc[k]: the slot matched, -1 for a new landmark, -2 dropped."""
        obs = _f64(obs).reshape(-1, 3)
        self._assoc = np.empty(obs.shape[0], dtype=np.int32)
        check(self._lib.slam_ekfslam_observe(self._h, int(obs.shape[0]), dptr(obs),
                                             self._assoc.ctypes.data_as(C.POINTER(C.c_int32))),
              "slam_ekfslam_observe")
        return self._assoc.copy()

    @property
    def count(self):
        c = C.c_int32(0)
        check(self._lib.slam_ekfslam_get_count(self._h, C.byref(c)), "slam_ekfslam_get_count")
        return c.value

    def set_count(self, count):
        """With set_state, places a state: the caller keeps the tail at zero."""
        check(self._lib.slam_ekfslam_set_count(self._h, int(count)), "slam_ekfslam_set_count")

    def landmarks(self):
        """(mean [count][3], cov [count][3][3]) of the landmarks held."""
        cnt = self.count
        mean = self.get_state(with_cov=False)[3:3 + 3 * cnt].reshape(cnt, 3)
        cov = np.empty((cnt, 3, 3))
        if cnt:
            rows = self.get_rows(np.arange(3, 3 + 3 * cnt))
            for j in range(cnt):
                cov[j] = rows[3 * j:3 * j + 3, 3 + 3 * j:6 + 3 * j]
        return mean, cov

    def pose(self):
        """(mu_r (3,), P_rr (3, 3))."""
        return self.get_state(with_cov=False)[:3], self.get_rows([0, 1, 2])[:, :3]

    def last_assoc(self):
        return self._assoc.copy()

    def last_scores(self):
        """The last call's scores [k][count0] (``record_assoc=True``)."""
        s = self.assoc_info()
        out = np.empty((self._assoc.size, s["count0"]))
        check(self._lib.slam_ekfslam_get_scores(self._h, dptr(out)), "slam_ekfslam_get_scores")
        return out

    def assoc_info(self):
        s = _lib.EKFSLAMAssocInfo()
        check(self._lib.slam_ekfslam_assoc_info(self._h, C.byref(s)), "slam_ekfslam_assoc_info")
        return dict(n_act=s.n_act, tiles=s.tiles, count=s.count, count0=s.count0,
                    matched=s.matched, new=s.created, dropped=s.dropped)

    def assoc_timing(self):
        out = np.zeros(4)
        check(self._lib.slam_ekfslam_assoc_timing(self._h, dptr(out)), "slam_ekfslam_assoc_timing")
        return dict(scan_ms=out[0], assign_ms=out[1], update_ms=out[2], init_ms=out[3])

    def set_pruning(self, view_range=None, **kw):
        """Landmark evidence and removal (slam_ekfslam_set_pruning):
        ``set_pruning(view_range, view_angle=None, init=1, hit=1, miss=1,
        ev_max=2**31 - 1, remove_below=0)`` turns it on (every live slot starts
        at ``init``) or replaces the configuration; ``set_pruning(None)`` turns
        it off.  The pass runs at the end of every ``observe`` / ``step`` without
        ids, an empty scan included."""
        if self.association is None:
            raise ValueError("set_pruning needs association='ml'")
        if view_range is None:
            if kw:
                raise ValueError("set_pruning(None) takes no other argument")
            check(self._lib.slam_ekfslam_set_pruning(self._h, None), "slam_ekfslam_set_pruning")
            self.prune = None
            return
        cfg = prune_config(view_range, **kw)
        check(self._lib.slam_ekfslam_set_pruning(self._h, C.byref(cfg)), "slam_ekfslam_set_pruning")
        self.prune = cfg

    def evidence(self):
        """The evidence of every slot, [n_landmarks] int32; 0 at and above the count."""
        e = np.empty(self.n_lm, dtype=np.int32)
        check(self._lib.slam_ekfslam_get_evidence(self._h, e.ctypes.data_as(_lib._I32)),
              "slam_ekfslam_get_evidence")
        return e

    def set_evidence(self, ev):
        e = np.ascontiguousarray(ev, dtype=np.int32).reshape(self.n_lm)
        check(self._lib.slam_ekfslam_set_evidence(self._h, e.ctypes.data_as(_lib._I32)),
              "slam_ekfslam_set_evidence")

    def remove(self, slots):
        """Remove the landmarks in ``slots`` (strictly increasing, below the
        count) from mu, P and the evidence now; the survivors keep their order."""
        s = np.ascontiguousarray(slots, dtype=np.int32).ravel()
        check(self._lib.slam_ekfslam_remove(self._h, int(s.size), s.ctypes.data_as(_lib._I32)),
              "slam_ekfslam_remove")

    def prune_info(self):
        """The last pass or ``remove``: the count before it, landmarks removed,
        surviving slots moved, the first removed slot (-1: none) and the device
        ms of the evidence kernel and of the compaction."""
        s = _lib.EKFSLAMPruneInfo()
        check(self._lib.slam_ekfslam_prune_info(self._h, C.byref(s)), "slam_ekfslam_prune_info")
        return dict(count_before=s.count_before, removed=s.removed, moved=s.moved, first=s.first,
                    evidence_ms=s.evidence_ms, compact_ms=s.compact_ms)
