"""Particle-filter ensemble: a handle on libslam_hip's slam_pfb_* entry points.

``n_filters`` independent filters of ``n_particles`` (<= 8192) particles each
on one GPU -- Monte-Carlo repetitions over seeds or maps, parameter sweeps, one
filter per robot.  One workgroup runs one filter's whole step; a ``run`` of any
number of steps is one launch.  Arrays carry a leading filter axis.
"""
from __future__ import annotations

import ctypes as C
from collections.abc import Sequence

import numpy as np

from . import _lib
from ._lib import PFConfig, PFResult, check, dptr
from .pf import DeviceParticleFilter, _f64, make_config

MAX_PARTICLES = 8192


def _per_filter(name, value, n_filters, shape):
    """``value`` as an array of shape (n_filters,) + shape: one ``shape`` (or a
    scalar) is broadcast to every filter, a leading ``n_filters`` axis is taken
    per filter; anything else raises ValueError."""
    a = np.asarray(value, dtype=np.float64)
    if a.ndim == 0 and len(shape) == 2:          # a scalar covariance: that variance on the diagonal
        a = a * np.eye(shape[0])
    if a.shape == (n_filters,) + shape:
        return a
    if a.shape == shape or a.ndim == 0:
        return np.broadcast_to(a, (n_filters,) + shape)
    raise ValueError(f"{name}: shape {a.shape} is neither {shape} (one value for every filter) "
                     f"nor {(n_filters,) + shape} (one per filter)")


def ensemble_configs(n_filters, n_particles, *, dt=0.1, q=None, r=None, x0=(10.0, 0.0, np.pi / 2),
                     motion="linear", likelihood="product", alphas=(0.1,) * 6, ess_threshold=None,
                     seed=0):
    """The ensemble's slam_pf_config array (pure Python: no device needed).
    ``q`` (3x3), ``r`` (2x2), ``alphas`` (6), ``x0`` (3), ``ess_threshold`` and
    ``seed`` take one value for every filter or a leading ``n_filters`` axis;
    ``motion``, ``likelihood`` and ``dt`` are shared."""
    B = int(n_filters)
    if B < 1:
        raise ValueError("n_filters must be >= 1")
    if not isinstance(motion, str) or not isinstance(likelihood, str) or np.ndim(dt) != 0:
        raise ValueError("motion, likelihood and dt are shared by the ensemble (scalars only)")
    q = np.diag([0.03, 0.03, np.deg2rad(2.0)]) ** 2 if q is None else q
    r = np.diag([0.3, 0.3]) ** 2 if r is None else r
    ess = n_particles / 100.0 if ess_threshold is None else ess_threshold
    qs = _per_filter("q", q, B, (3, 3))
    rs = _per_filter("r", r, B, (2, 2))
    als = _per_filter("alphas", alphas, B, (6,))
    x0s = _per_filter("x0", x0, B, (3,))
    ths = _per_filter("ess_threshold", ess, B, ())
    sd = np.asarray(seed)
    if sd.shape == (B,):
        seeds = [int(v) for v in sd]
    elif sd.ndim == 0:
        seeds = [int(sd)] * B
    else:
        raise ValueError(f"seed: shape {sd.shape} is neither a scalar nor ({B},)")
    cfgs = (PFConfig * B)()
    for b in range(B):
        c = make_config(n_particles, dt=dt, q=qs[b], r=rs[b], x0=x0s[b], motion=motion,
                        likelihood=likelihood, alphas=als[b], ess_threshold=float(ths[b]),
                        seed=seeds[b])
        C.memmove(C.byref(cfgs[b]), C.byref(c), C.sizeof(PFConfig))
    return cfgs


class BatchRunResults(Sequence):
    """The records of an ensemble run, indexable as ``[step][filter]`` over the
    returned slam_pf_result array; a record becomes the dict of
    DeviceParticleFilter._res when it is accessed.  ``records`` is the same
    memory as a NumPy structured array of shape (n_steps, n_filters)."""

    def __init__(self, res, n_steps, n_filters, dicts=None):
        self._r, self._k, self._b, self._d = res, int(n_steps), int(n_filters), dicts

    @property
    def records(self):
        if self._r is None:
            raise AttributeError("records: this run was returned as dicts (confirm_ess)")
        return np.ctypeslib.as_array(self._r).reshape(self._k, self._b)

    def __len__(self):
        return self._k

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self._k))]
        if i < 0:
            i += self._k
        if not 0 <= i < self._k:
            raise IndexError(i)
        if self._d is not None:
            return self._d[i]
        return _StepRow(self._r, i * self._b, self._b)


class _StepRow(Sequence):
    def __init__(self, res, base, n):
        self._r, self._base, self._n = res, base, n

    def __len__(self):
        return self._n

    def __getitem__(self, b):
        if isinstance(b, slice):
            return [self[j] for j in range(*b.indices(self._n))]
        if b < 0:
            b += self._n
        if not 0 <= b < self._n:
            raise IndexError(b)
        return DeviceParticleFilter._res(self._r[self._base + b])


class BatchParticleFilter:
    """``n_filters`` particle filters on one GPU.  Keywords as
    DeviceParticleFilter's (see ensemble_configs for the per-filter ones);
    ``landmarks``: (NL, 2) for every filter or (n_filters, NL, 2)."""

    ESS_CONFIRM_BAND = 1e-9

    def __init__(self, n_filters, n_particles, landmarks, *, device=0, **kw):
        self.n_filters = B = int(n_filters)
        self.n = int(n_particles)
        lm = np.asarray(landmarks, dtype=np.float64)
        if lm.ndim == 2:
            lm = np.broadcast_to(lm, (B,) + lm.shape)
        if lm.ndim != 3 or lm.shape[0] != B or lm.shape[2] != 2:
            raise ValueError(f"landmarks: shape {lm.shape} is neither (NL, 2) nor ({B}, NL, 2)")
        self.lm = np.ascontiguousarray(lm)
        self.nl = self.lm.shape[1]
        self.cfgs = ensemble_configs(B, self.n, **kw)
        self.ess_threshold = np.array([c.ess_threshold for c in self.cfgs])
        self.motion = kw.get("motion", "linear")
        lib = _lib.load()
        h = C.c_void_p()
        check(lib.slam_pfb_create(self.cfgs, B, self.n, self.nl, dptr(self.lm), int(device),
                                  C.byref(h)), "slam_pfb_create")
        self._h, self._lib = h, lib
        self.resample_next = np.zeros(B, dtype=bool)
        self._z_steps = 0

    # ------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._lib.slam_pfb_destroy(self._h)
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
    def set_state(self, x=None, y=None, th=None, w=None):
        shape = (self.n_filters, self.n)
        arrs = [None if a is None else _f64(a, shape) for a in (x, y, th, w)]
        check(self._lib.slam_pfb_set_state(self._h, *[dptr(a) for a in arrs]), "slam_pfb_set_state")
        if w is not None:
            ww = arrs[3]
            # the reference's own dot decides (particle_filter.py:210-211)
            rn = np.array([1.0 / float(r @ r) < t for r, t in zip(ww, self.ess_threshold)])
            self.set_resample_next(rn)

    def get_state(self):
        out = [np.empty((self.n_filters, self.n)) for _ in range(4)]
        check(self._lib.slam_pfb_get_state(self._h, *[dptr(a) for a in out]), "slam_pfb_get_state")
        return tuple(out)

    def get_weights_raw(self):
        """(w_un [B][NP], s [B]): the last step's weights before normalisation
        and the np.sum each filter divided them by."""
        w = np.empty((self.n_filters, self.n))
        s = np.empty(self.n_filters)
        check(self._lib.slam_pfb_get_weights_raw(self._h, dptr(w), dptr(s)),
              "slam_pfb_get_weights_raw")
        return w, s

    def set_resample_next(self, flags):
        """Per-filter decision of the next step's resample; -1 keeps the device's."""
        f = np.ascontiguousarray(np.broadcast_to(np.asarray(flags), (self.n_filters,)), dtype=np.int32)
        check(self._lib.slam_pfb_set_resample_next(self._h, f.ctypes.data_as(_lib._I32)),
              "slam_pfb_set_resample_next")
        self.resample_next = np.where(f >= 0, f != 0, self.resample_next)

    def set_ess_band(self, band):
        check(self._lib.slam_pfb_set_ess_band(self._h, float(band)), "slam_pfb_set_ess_band")
        self.ESS_CONFIRM_BAND = float(band)

    # ---------------------------------------------------------------- step
    def _confirm_ess(self, outs):
        """DeviceParticleFilter._confirm_ess for the flagged filters only: the
        reference's `1 / (pw @ pw.T)` re-formed on the host where the device's
        ESS lies within the band of ESS_TH, the decisions handed back."""
        near = [b for b, o in enumerate(outs) if o["ess_near"]]
        for o in outs:
            o["ess_confirmed"] = False
        if not near:
            return outs
        w = self.get_state()[3]
        flags = np.full(self.n_filters, -1, dtype=np.int32)
        for b in near:
            pw = w[b].reshape(1, -1)
            ess = float(np.reciprocal(pw @ pw.T)[0, 0])
            rn = ess < self.ess_threshold[b]
            if rn != bool(outs[b]["resample_next"]):
                flags[b] = int(rn)
            outs[b].update(resample_next=bool(rn), ess_host=ess, ess_confirmed=True)
        if (flags >= 0).any():
            self.set_resample_next(flags)
        return outs

    def _after(self, outs, raise_on_clamp):
        self.resample_next = np.array([o["resample_next"] for o in outs])
        if raise_on_clamp:
            bad = [b for b, o in enumerate(outs) if o["status"] & 1]
            if bad:
                raise IndexError(f"filters {bad}: resample position beyond the last cumulative "
                                 "weight (IndexError in particle_filter.py:219)")

    def step(self, control, z, noise=None, u_resample=None, raise_on_clamp=False):
        """One step of every filter -> list of DeviceParticleFilter._res dicts.
        control (2,) or [B][2]; z [B][NL][2]; noise [B][NP][3] or None (device
        RNG); u_resample [B] or None (NaN / None: device RNG)."""
        B = self.n_filters
        ctl = np.ascontiguousarray(np.broadcast_to(np.asarray(control, dtype=np.float64), (B, 2)))
        zz = _f64(z, (B, self.nl, 2))
        nz = None if noise is None else _f64(noise, (B, self.n, 3))
        u = None if u_resample is None else _f64(np.broadcast_to(
            np.asarray(u_resample, dtype=np.float64), (B,)))
        res = (PFResult * B)()
        check(self._lib.slam_pfb_step(self._h, dptr(ctl), dptr(zz), dptr(nz), dptr(u), res),
              "slam_pfb_step")
        outs = [DeviceParticleFilter._res(r) for r in res]
        self._confirm_ess(outs)
        self._after(outs, raise_on_clamp)
        return outs

    def resample_indices(self, u_resample=None):
        """Exact systematic-resampling indices of the current weights, [B][NP]."""
        B = self.n_filters
        u = None if u_resample is None else _f64(np.broadcast_to(
            np.asarray(u_resample, dtype=np.float64), (B,)))
        idx = np.empty((B, self.n), dtype=np.int64)
        check(self._lib.slam_pfb_resample_indices(self._h, dptr(u), idx.ctypes.data_as(_lib._I64)),
              "slam_pfb_resample_indices")
        return idx

    # ------------------------------------------------------ device-resident
    def load_observations(self, z_all):
        z_all = _f64(z_all).reshape(-1, self.n_filters, self.nl, 2)
        check(self._lib.slam_pfb_load_observations(self._h, z_all.shape[0], dptr(z_all)),
              "slam_pfb_load_observations")
        self._z_steps = z_all.shape[0]

    def run(self, first_step, controls, want_results=True, confirm_ess=False, raise_on_clamp=False):
        """Steps [first_step, first_step + K) from the loaded observations in one
        launch (device RNG, no host round trip between steps).  controls:
        (K, 2) for every filter or (K, B, 2).  ``confirm_ess=True``: one step
        per launch, ess_near filters confirmed on the host in between."""
        B = self.n_filters
        c = np.asarray(controls, dtype=np.float64)
        if c.ndim == 2:
            c = np.broadcast_to(c[:, None, :], (c.shape[0], B, 2))
        c = np.ascontiguousarray(c.reshape(-1, B, 2))
        k = c.shape[0]
        if confirm_ess:
            rows = []
            for i in range(k):
                res = (PFResult * B)()
                check(self._lib.slam_pfb_run(self._h, int(first_step) + i, 1, dptr(c[i:i + 1]), res),
                      "slam_pfb_run")
                outs = [DeviceParticleFilter._res(r) for r in res]
                self._confirm_ess(outs)
                self._after(outs, raise_on_clamp)
                rows.append(outs)
            return BatchRunResults(None, k, B, rows) if want_results else None
        res = (PFResult * (k * B))()
        check(self._lib.slam_pfb_run(self._h, int(first_step), k, dptr(c), res), "slam_pfb_run")
        out = BatchRunResults(res, k, B)
        rec = out.records
        self.resample_next = rec["resample_next"][-1] != 0
        if raise_on_clamp and (rec["status"] & 1).any():
            bad = sorted(set(np.nonzero(rec["status"] & 1)[1].tolist()))
            raise IndexError(f"filters {bad}: resample position beyond the last cumulative "
                             "weight (IndexError in particle_filter.py:219)")
        return out if want_results else None

    def timing(self):
        """(ms, launches) of the last step / run call (HIP events)."""
        ms, cnt = C.c_double(0.0), C.c_int64(0)
        check(self._lib.slam_pfb_timing(self._h, C.byref(ms), C.byref(cnt)), "slam_pfb_timing")
        return ms.value, cnt.value
