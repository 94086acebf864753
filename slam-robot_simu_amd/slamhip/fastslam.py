"""Device FastSLAM 1.0 (known data association, or per-particle
maximum-likelihood association) and 2.0 (known association, poses drawn from
the observation-informed proposal): a handle on libslam_hip's slam_fs_* entry
points.

Every particle carries a pose, a weight and one 2-D EKF (mean, symmetric 2 x 2
covariance) per landmark, resident in HBM; a step observes any subset of the
landmarks as (range, bearing, orientation) triples with their ids -- what
``ScanSensor.scan`` returns.  Resampling, prediction and the step end are the
single particle filter's (slamhip.pf); the per-particle map update with its
log-domain weights and the resampling gather of whole maps are this handle's
own kernels (csrc/fastslam.inl).

With ``association="ml"`` the observations carry no ids: every particle scores
an observation against the landmarks of its own map, takes the likeliest (or
starts a new landmark when none reaches ``p_new``), and ``n_landmarks`` is the
capacity of every particle's map (include/slam_hip.h states the contract).

With ``proposal="measurement"`` (FastSLAM 2.0; known association and linear
motion) a step filters every particle's pose through the scan before drawing
it: the pose comes from N(mu, Sigma) with the scan's seen landmarks folded in,
and the weight no longer depends on the draw.  ``noise`` is then three
standard normals per particle, not Q-shaped noise.

With ``association="ml_marginal"`` (which needs ``proposal="measurement"``)
the two go together, FastSLAM 2.0 without ids: every particle associates
inside its proposal, the score of a candidate marginalising the pose
uncertainty the proposal still has; ``n_landmarks`` is again the capacity.

Either associating kind can prune (``prune=dict(view_range=...)``): every
landmark carries an evidence counter, raised when an observation matches it and
lowered when it lies in the sensor's view unmatched, and is removed from its
particle's map once the counter falls below a threshold (the contract is in
include/slam_hip.h, the kernel fs_prune_kernel).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (FSAssocConfig, FSConfig, FSProposalConfig, FSPruneConfig, PFResult, check,
                   dptr)
from .pf import DeviceParticleFilter, RunResults, _f64, make_config


# The likelihood below which an observation starts a new landmark
# (association="ml"); chosen by the sweep recorded in DESIGN 11c.
P_NEW_DEFAULT = 1e-4


def _ids_obs(ids, obs):
    if ids is None:
        return None, np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, 3)
    ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
    obs = np.ascontiguousarray(obs, dtype=np.float64).reshape(-1, 3)
    if obs.shape[0] != ids.size:
        raise ValueError("ids and obs disagree in length")
    return ids, obs


def _iptr(ids):
    return None if ids is None else ids.ctypes.data_as(_lib._I64)


def prune_config(view_range, view_angle=None, init=1, hit=1, miss=1, ev_max=2 ** 31 - 1,
                 remove_below=0):
    """slam_fs_prune_config from the front end's keywords.  ``view_angle`` is
    the half-angle of the sensor's fan as ScanSensor takes it (None: range
    only); the C-ABI gets tan(pi/2 - view_angle)."""
    c = FSPruneConfig()
    c.view_range = float(view_range)
    c.use_angle = int(view_angle is not None)
    c.view_tan = float(np.tan(np.pi / 2 - view_angle)) if c.use_angle else 0.0
    c.init, c.hit, c.miss = int(init), int(hit), int(miss)
    c.ev_max, c.remove_below = int(ev_max), int(remove_below)
    return c


class DeviceFastSLAM:
    """Particles with per-particle landmark maps on one GPU.

    ``noise`` = (r_dist, r_dir, r_orient): ScanSensor's range noise fraction and
    its bearing / orientation sigmas (rad).  ``association``: "known" (ids with
    every observation) or "ml" (per-particle maximum likelihood: ``ids`` is
    None everywhere, ``n_landmarks`` is the capacity of a particle's map,
    ``p_new`` the likelihood below which an observation starts a new landmark,
    ``record_assoc`` keeps each update's choices for ``last_assoc``), or
    "ml_marginal" (the same without ids under ``proposal="measurement"``,
    which it requires: the score folds the proposal's pose covariance into S;
    ``last_assoc`` works whatever ``record_assoc`` says).
    ``proposal``: "motion" (FastSLAM 1.0: the pose from the motion model) or
    "measurement" (FastSLAM 2.0: the pose from the proposal that has seen the
    scan; ``step``'s ``noise`` is then [NP][3] standard normals, ``predict`` and
    ``update`` raise, ``record_proposal`` keeps each step's mean, covariance
    and log weight for ``last_proposal``).  ``prune``: None, or ``set_pruning``'s
    keywords as a dict (associating handles only): landmarks carry an evidence
    counter and those the scans stop supporting are removed.  The other
    keywords are DeviceParticleFilter's."""

    ESS_CONFIRM_BAND = DeviceParticleFilter.ESS_CONFIRM_BAND

    def __init__(self, n_particles, n_landmarks, *, dt=0.1, q=None, alphas=(0.1,) * 6,
                 x0=(10.0, 0.0, np.pi / 2), motion="linear",
                 noise=(0.1, np.deg2rad(3.0), np.deg2rad(3.0)), use_orient=True,
                 ess_threshold=None, seed=0, device=0, association="known",
                 p_new=P_NEW_DEFAULT, record_assoc=False, proposal="motion",
                 record_proposal=False, prune=None):
        if association not in ("known", "ml", "ml_marginal"):
            raise ValueError("association: 'known', 'ml' or 'ml_marginal'")
        if prune is not None and association == "known":
            raise ValueError("prune needs association='ml' or 'ml_marginal'")
        if proposal not in _lib.FS_PROPOSAL:
            raise ValueError("proposal: 'motion' or 'measurement'")
        if proposal == "measurement" and association == "ml":
            raise ValueError("proposal='measurement' needs association='known' or 'ml_marginal' "
                             "(the score that marginalises the pose)")
        if association == "ml_marginal" and proposal != "measurement":
            raise ValueError("association='ml_marginal' needs proposal='measurement'")
        lib = _lib.load()
        self.n = int(n_particles)
        self.nl = int(n_landmarks)
        cfg = FSConfig()
        cfg.pf = make_config(self.n, dt=dt, q=q, x0=x0, motion=motion, alphas=alphas,
                             ess_threshold=ess_threshold, seed=seed)
        cfg.r_dist, cfg.r_dir, cfg.r_orient = (float(v) for v in noise)
        cfg.use_orient = int(bool(use_orient))
        self.cfg = cfg
        self.motion = motion
        self.association = association
        self.record_assoc = bool(record_assoc)
        self.proposal = proposal
        self.record_proposal = bool(record_proposal)
        self._last_k = 0
        h = C.c_void_p()
        if association in ("ml", "ml_marginal"):
            if not p_new > 0:
                raise ValueError("p_new must be positive")
            acfg = FSAssocConfig(float(np.log(p_new)), int(self.record_assoc), 0)
            self.acfg = acfg
        if association == "ml":
            check(lib.slam_fs_create_assoc(C.byref(cfg), C.byref(acfg), self.n, self.nl, int(device),
                                           C.byref(h)), "slam_fs_create_assoc")
        elif association == "ml_marginal":
            pcfg = FSProposalConfig(int(self.record_proposal), 0)
            check(lib.slam_fs_create_assoc_proposal(C.byref(cfg), C.byref(acfg), C.byref(pcfg),
                                                    self.n, self.nl, int(device), C.byref(h)),
                  "slam_fs_create_assoc_proposal")
        elif proposal == "measurement":
            pcfg = FSProposalConfig(int(self.record_proposal), 0)
            check(lib.slam_fs_create_proposal(C.byref(cfg), C.byref(pcfg), self.n, self.nl,
                                              int(device), C.byref(h)), "slam_fs_create_proposal")
        else:
            check(lib.slam_fs_create(C.byref(cfg), self.n, self.nl, int(device), C.byref(h)),
                  "slam_fs_create")
        self._h = h
        self._lib = lib
        self.resample_next = False
        self.last = None
        self._run_steps = 0
        self._run_counts = np.zeros(0, dtype=np.int32)
        self.prune = None
        if prune is not None:
            try:
                self.set_pruning(**prune)
            except Exception:
                self.close()
                raise

    # ------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._lib.slam_fs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # --------------------------------------------------------------- state
    def info(self):
        n, nl, ns = C.c_int64(0), C.c_int32(0), C.c_int32(0)
        check(self._lib.slam_fs_info(self._h, C.byref(n), C.byref(nl), C.byref(ns)), "slam_fs_info")
        return dict(n_particles=n.value, n_landmarks=nl.value, n_seen=ns.value)

    def set_state(self, x=None, y=None, th=None, w=None):
        arrs = [None if a is None else _f64(a, (self.n,)) for a in (x, y, th, w)]
        check(self._lib.slam_fs_set_state(self._h, *[dptr(a) for a in arrs]), "slam_fs_set_state")
        if w is not None:
            ww = arrs[3]
            self.set_resample_next(bool(1.0 / float(ww @ ww) < self.cfg.pf.ess_threshold))

    def get_state(self):
        out = [np.empty(self.n) for _ in range(4)]
        check(self._lib.slam_fs_get_state(self._h, *[dptr(a) for a in out]), "slam_fs_get_state")
        return tuple(out)

    def set_resample_next(self, on):
        check(self._lib.slam_fs_set_resample_next(self._h, int(bool(on))),
              "slam_fs_set_resample_next")
        self.resample_next = bool(on)

    def set_maps(self, seen, mean, cov):
        """seen [NL], mean [NP][NL][2], cov [NP][NL][3] (pxx, pxy, pyy).
        association="ml": ``seen`` is ignored (None will do); the counts say
        which slots hold (``set_counts``)."""
        if seen is None:
            seen = np.zeros(self.nl, dtype=np.int32)
        seen = np.ascontiguousarray(seen, dtype=np.int32).reshape(self.nl)
        mean = _f64(mean, (self.n, self.nl, 2))
        cov = _f64(cov, (self.n, self.nl, 3))
        check(self._lib.slam_fs_set_maps(self._h, seen.ctypes.data_as(_lib._I32), dptr(mean),
                                         dptr(cov)), "slam_fs_set_maps")

    def get_maps(self):
        """(seen, mean, cov) of every particle; unseen landmarks are NaN."""
        seen = np.empty(self.nl, dtype=np.int32)
        mean = np.empty((self.n, self.nl, 2))
        cov = np.empty((self.n, self.nl, 3))
        check(self._lib.slam_fs_get_maps(self._h, seen.ctypes.data_as(_lib._I32), dptr(mean),
                                         dptr(cov)), "slam_fs_get_maps")
        return seen, mean, cov

    def get_map(self, particle):
        """(seen, mean [NL][2], cov [NL][3]) of one particle, O(NL)."""
        seen = np.empty(self.nl, dtype=np.int32)
        mean = np.empty((self.nl, 2))
        cov = np.empty((self.nl, 3))
        check(self._lib.slam_fs_get_map(self._h, int(particle), seen.ctypes.data_as(_lib._I32),
                                        dptr(mean), dptr(cov)), "slam_fs_get_map")
        return seen, mean, cov

    def set_counts(self, counts):
        """association="ml": the landmarks each particle holds, [NP] in [0, n_landmarks]."""
        c = np.ascontiguousarray(counts, dtype=np.int32).reshape(self.n)
        check(self._lib.slam_fs_set_counts(self._h, c.ctypes.data_as(_lib._I32)),
              "slam_fs_set_counts")

    def get_counts(self):
        c = np.empty(self.n, dtype=np.int32)
        check(self._lib.slam_fs_get_counts(self._h, c.ctypes.data_as(_lib._I32)),
              "slam_fs_get_counts")
        return c

    def last_assoc(self):
        """association="ml", record_assoc=True: the last update's choices,
        [k][NP]: the slot matched, -1 a new landmark, -2 dropped (map full)."""
        a = np.empty((self._last_k, self.n), dtype=np.int32)
        check(self._lib.slam_fs_get_assoc(self._h, a.ctypes.data_as(_lib._I32)),
              "slam_fs_get_assoc")
        return a

    def set_pruning(self, view_range=None, **kw):
        """Landmark evidence and removal on an associating handle
        (slam_fs_set_pruning): ``set_pruning(view_range, view_angle=None,
        init=1, hit=1, miss=1, ev_max=2**31 - 1, remove_below=0)`` turns it on
        (every live slot starts at ``init``) or replaces the configuration;
        ``set_pruning(None)`` turns it off.  A landmark gains ``hit`` when an
        observation matches it, loses ``miss`` when it lies within
        ``view_range`` (and the fan of half-angle ``view_angle``) of the
        particle unmatched, and is removed below ``remove_below``."""
        if self.association == "known":
            raise ValueError("set_pruning needs association='ml' or 'ml_marginal'")
        if view_range is None:
            if kw:
                raise ValueError("set_pruning(None) takes no other argument")
            check(self._lib.slam_fs_set_pruning(self._h, None), "slam_fs_set_pruning")
            self.prune = None
            return
        cfg = prune_config(view_range, **kw)
        check(self._lib.slam_fs_set_pruning(self._h, C.byref(cfg)), "slam_fs_set_pruning")
        self.prune = cfg

    def evidence(self):
        """The evidence of every slot, [NP][n_landmarks] int32; 0 at and above a
        particle's count."""
        e = np.empty((self.n, self.nl), dtype=np.int32)
        check(self._lib.slam_fs_get_evidence(self._h, e.ctypes.data_as(_lib._I32)),
              "slam_fs_get_evidence")
        return e

    def set_evidence(self, ev):
        e = np.ascontiguousarray(ev, dtype=np.int32).reshape(self.n, self.nl)
        check(self._lib.slam_fs_set_evidence(self._h, e.ctypes.data_as(_lib._I32)),
              "slam_fs_set_evidence")

    def last_removed(self):
        """The landmarks the last step's pass removed, per particle [NP]."""
        r = np.empty(self.n, dtype=np.int32)
        check(self._lib.slam_fs_get_removed(self._h, r.ctypes.data_as(_lib._I32)),
              "slam_fs_get_removed")
        return r

    def last_proposal(self):
        """proposal="measurement", record_proposal=True: the last step's
        proposal before sampling -- mean [NP][3], covariance [NP][6] (00 01 02
        11 12 22) and log weight L [NP]."""
        mean, cov, L = np.empty((self.n, 3)), np.empty((self.n, 6)), np.empty(self.n)
        check(self._lib.slam_fs_get_proposal(self._h, dptr(mean), dptr(cov), dptr(L)),
              "slam_fs_get_proposal")
        return mean, cov, L

    def best_map(self):
        """The map estimate: the map of the last step's heaviest particle, as
        x_est is its pose."""
        if self.last is None:
            raise RuntimeError("best_map: no step has run yet")
        return self.get_map(self.last["max_idx"])

    # ---------------------------------------------------------------- step
    def _confirm_ess(self, out):
        """DeviceParticleFilter._confirm_ess: an ess_near step's resample
        decision re-formed on the host by the reference's own expression."""
        th = self.cfg.pf.ess_threshold
        out["ess_confirmed"] = False
        if not abs(out["ess"] - th) <= self.ESS_CONFIRM_BAND * th:
            return out
        pw = self.get_state()[3]
        ess = float(np.reciprocal(pw @ pw.T))
        rn = ess < th
        if rn != bool(out["resample_next"]):
            self.set_resample_next(rn)
        out.update(resample_next=rn, ess_host=ess, ess_confirmed=True)
        self.resample_next = rn
        return out

    def _finish(self, res):
        out = DeviceParticleFilter._res(res)
        self.resample_next = out["resample_next"]
        self._confirm_ess(out)
        self.last = out
        return out

    def step(self, control, ids, obs, noise=None, u_resample=float("nan")):
        ctl = _f64(control, (2,))
        ids, obs = _ids_obs(ids, obs)
        nz = None if noise is None else _f64(noise, (self.n, 3))
        res = PFResult()
        check(self._lib.slam_fs_step(self._h, dptr(ctl), obs.shape[0], _iptr(ids), dptr(obs),
                                     dptr(nz), float(u_resample), C.byref(res)), "slam_fs_step")
        self._last_k = obs.shape[0]
        return self._finish(res)

    def resample(self, u_resample=float("nan"), force=False):
        flag = C.c_int32(0)
        check(self._lib.slam_fs_resample(self._h, float(u_resample), int(bool(force)),
                                         C.byref(flag)), "slam_fs_resample")
        if flag.value:
            self.resample_next = False
        return bool(flag.value)

    def predict(self, control, noise=None):
        ctl = _f64(control, (2,))
        nz = None if noise is None else _f64(noise, (self.n, 3))
        check(self._lib.slam_fs_predict(self._h, dptr(ctl), dptr(nz)), "slam_fs_predict")

    def update(self, ids, obs):
        ids, obs = _ids_obs(ids, obs)
        res = PFResult()
        check(self._lib.slam_fs_update(self._h, obs.shape[0], _iptr(ids), dptr(obs), C.byref(res)),
              "slam_fs_update")
        self._last_k = obs.shape[0]
        return self._finish(res)

    # ------------------------------------------------------- multi-step run
    def load_observations(self, steps):
        """steps: a sequence of (ids, obs) per step, uploaded once."""
        pairs = [_ids_obs(i, o) for i, o in steps]
        counts = np.array([o.shape[0] for _, o in pairs], dtype=np.int32)
        if any(i is None for i, _ in pairs):
            if not all(i is None for i, _ in pairs):
                raise ValueError("ids: None for every step or for none")
            ids = None
        else:
            ids = np.ascontiguousarray(np.concatenate([i for i, _ in pairs] + [np.zeros(0, np.int64)]))
        obs = np.ascontiguousarray(np.concatenate([o for _, o in pairs] + [np.zeros((0, 3))]))
        check(self._lib.slam_fs_load_observations(self._h, len(pairs),
                                                  counts.ctypes.data_as(_lib._I32),
                                                  _iptr(ids), dptr(obs)),
              "slam_fs_load_observations")
        self._run_steps = len(pairs)
        self._run_counts = counts

    def run(self, first_step, controls):
        """Steps [first_step, first_step + len(controls)) of the loaded
        observations with the device RNG; the records of ``step`` in turn."""
        controls = _f64(controls).reshape(-1, 2)
        k = controls.shape[0]
        res = (PFResult * k)()
        check(self._lib.slam_fs_run(self._h, int(first_step), k, dptr(controls), res), "slam_fs_run")
        self.resample_next = bool(res[k - 1].resample_next)
        self._last_k = int(self._run_counts[int(first_step) + k - 1])
        self.last = DeviceParticleFilter._res(res[k - 1])
        return RunResults(res)

    def timing(self):
        """HIP-event ms of the last step's {map gather, predict, map update +
        weights, step end}; with proposal="measurement" one launch does the
        motion, the proposal, the sampling and the map update ("predict"), and
        "map_update" is the weights alone."""
        out = np.zeros(4)
        check(self._lib.slam_fs_timing(self._h, dptr(out)), "slam_fs_timing")
        return dict(zip(("map_gather", "predict", "map_update", "step_end"), out.tolist()))
