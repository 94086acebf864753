"""NumPy restatement of FastSLAM 1.0 with per-particle maximum-likelihood data
association -- the test oracle of an associating slam_fs handle
(include/slam_hip.h states the same contract).

Only the association is new: ``wrap``, ``scan_r``, ``init_landmark`` and
``update_landmark`` are fastslam_ref's, resampling and the step end are
pf_oracle's.  ``FSDARef`` is vectorised over particles and slots for a dtype
parameter (float64, and np.longdouble to measure float64's own rounding);
``update_loop`` is the same update as a plain per-particle Python loop on
``update_landmark_generic``, which the vectorised form is checked against.
Per step it also returns the association matrix and every decision's margin:
``|l_best - log_p_new|``, and ``l_best - l_second`` as well where the best
candidate is taken; infinite where there is no candidate.
Test infrastructure only: the shipped path never imports it.
"""
from __future__ import annotations

import numpy as np

import fastslam_ref as fr
import pf_oracle as po

NEW, DROPPED = -1, -2


class FSDARef:
    """State and one step of the associating filter, in ``dtype``.  Particle p
    holds ``cnt[p]`` landmarks in slots 0..cnt[p]-1 of ``mean`` / ``cov``
    ([n][cap][2], [n][cap][3]); the slots above are NaN."""

    def __init__(self, n, cap, *, p_new=0.1, dt=0.1, motion="linear", alphas=(0.1,) * 6,
                 noise=(0.1, np.deg2rad(3.0), np.deg2rad(3.0)), use_orient=True, ess_th=None,
                 x0=(10.0, 0.0, np.pi / 2), dtype=np.float64):
        self.n, self.cap, self.dt, self.motion, self.alphas = n, cap, dt, motion, tuple(alphas)
        self.r_dist, self.r_dir, self.r_orient = noise
        self.use_orient = use_orient
        self.ess_th = n / 100.0 if ess_th is None else ess_th
        self.t = dtype
        self.log_p_new = float(np.log(p_new))       # the double the handle is given
        self.x = np.full(n, x0[0], dtype=dtype)
        self.y = np.full(n, x0[1], dtype=dtype)
        self.th = np.full(n, x0[2], dtype=dtype)
        self.w = np.full(n, 1 / n, dtype=dtype)
        self.cnt = np.zeros(n, dtype=np.int32)
        self.mean = np.full((n, cap, 2), np.nan, dtype=dtype)
        self.cov = np.full((n, cap, 3), np.nan, dtype=dtype)

    def load(self, other):
        """Take another instance's state (cast to this dtype)."""
        for k in ("x", "y", "th", "w", "mean", "cov"):
            setattr(self, k, getattr(other, k).astype(self.t))
        self.cnt = other.cnt.copy()

    def snapshot(self):
        return dict(x=self.x.copy(), y=self.y.copy(), th=self.th.copy(), w=self.w.copy(),
                    cnt=self.cnt.copy(), mean=self.mean.copy(), cov=self.cov.copy())

    def needs_resample(self):
        return po.ess_of(self.w) < self.ess_th

    # ------------------------------------------------------------ the stages
    def _resample(self, ofs, out):
        idx = po.systematic_indices(self.w, self.t(ofs))
        if (idx < 0).any():
            raise IndexError("resample position beyond the last cumulative weight")
        out["idx"] = idx
        self.x, self.y, self.th = self.x[idx], self.y[idx], self.th[idx]
        self.mean, self.cov, self.cnt = self.mean[idx], self.cov[idx], self.cnt[idx]
        self.w = np.full(self.n, 1 / self.n, dtype=self.t)

    def _predict(self, control, noise):
        t = self.t
        v, om = control
        noise = np.asarray(noise).astype(t)
        if self.motion == "linear":
            xn, yn, tn = po.motion_linear(self.x, self.y, self.th, self.dt, v, om)
            self.x, self.y, self.th = xn + noise[:, 0], yn + noise[:, 1], tn.astype(t) + noise[:, 2]
        else:
            xn, yn, tn = po.motion_velocity(self.x, self.y, self.th, v, om, self.dt, self.alphas,
                                            noise)
            self.x, self.y, self.th = xn, yn, tn.astype(t)

    def associate_update(self, obs):
        """The update of one step: returns (L [n], assoc [k][n], margin [k][n])."""
        t, n = self.t, self.n
        obs = np.asarray(obs, dtype=np.float64).reshape(-1, 3)
        k = obs.shape[0]
        psi_p = t(np.pi / 2) - self.th
        c, s = np.cos(psi_p), np.sin(psi_p)
        psi_w = fr.wrap(psi_p)
        lpn = t(self.log_p_new)
        ln2pi = np.log(2 * t(np.pi))
        cnt0 = self.cnt.copy()
        jm = int(cnt0.max()) if n else 0               # no slot at or above it is a candidate
        matched = np.zeros((n, jm), dtype=bool)
        below = np.arange(jm)[None, :] < cnt0[:, None]
        rows = np.arange(n)
        L = np.zeros(n, dtype=t)
        assoc = np.empty((k, n), dtype=np.int32)
        margin = np.full((k, n), np.inf)
        for q, z in enumerate(obs):
            d, phi, psi = (t(v_) for v_ in z)
            R0, R1 = fr.scan_r(d, t(self.r_dist), t(self.r_dir))
            if self.use_orient:
                e = fr.wrap(psi - psi_w)
                L -= e * e / (2 * (t(self.r_dir) ** 2 + t(self.r_orient) ** 2))
            allowed = below & ~matched
            has = allowed.any(axis=1)
            best = np.zeros(n, dtype=np.int64)
            lbest = np.full(n, -np.inf, dtype=t)
            if jm:
                with np.errstate(all="ignore"):
                    r = fr.update_landmark(self.x[:, None], self.y[:, None], c[:, None], s[:, None],
                                           self.mean[:, :jm, 0], self.mean[:, :jm, 1],
                                           self.cov[:, :jm, 0], self.cov[:, :jm, 1],
                                           self.cov[:, :jm, 2], d, phi, R0, R1)
                    lj = r[5] - ln2pi
                lj = np.where(allowed & ~np.isnan(lj), lj, -np.inf)
                best = np.argmax(lj, axis=1)               # the first of equal maxima: the lowest slot
                lbest = lj[rows, best]
                l2 = lj.copy()
                l2[rows, best] = -np.inf
                # the runner-up counts only where the best candidate is taken:
                # below log_p_new the outcome does not depend on which one is best
                with np.errstate(invalid="ignore"):
                    mg = np.abs(lbest - lpn)
                    mg = np.where(lbest < lpn, mg, np.minimum(mg, lbest - l2.max(axis=1)))
                margin[q, has] = mg[has].astype(np.float64)
            match = has & ~(lbest < lpn)
            new = ~match
            room = new & (self.cnt < self.cap)
            assoc[q] = np.where(match, best, np.where(room, NEW, DROPPED))
            L[new] += lpn
            L[match] += lbest[match]
            pm = np.flatnonzero(match)
            if pm.size:
                bm = best[pm]
                self.mean[pm, bm, 0], self.mean[pm, bm, 1] = r[0][pm, bm], r[1][pm, bm]
                self.cov[pm, bm, 0], self.cov[pm, bm, 1] = r[2][pm, bm], r[3][pm, bm]
                self.cov[pm, bm, 2] = r[4][pm, bm]
                matched[pm, bm] = True
            pr = np.flatnonzero(room)
            if pr.size:
                i = fr.init_landmark(self.x[pr], self.y[pr], c[pr], s[pr], d, phi, R0, R1)
                sl = self.cnt[pr]
                self.mean[pr, sl, 0], self.mean[pr, sl, 1] = i[0], i[1]
                self.cov[pr, sl, 0], self.cov[pr, sl, 1], self.cov[pr, sl, 2] = i[2], i[3], i[4]
                self.cnt[pr] += 1
        return L, assoc, margin

    def _step_end(self, L, out):
        w_un = self.w * np.exp(L - np.max(L)) if L.size else self.w
        out["weight_sum"] = float(np.sum(w_un.reshape(1, -1)))
        self.w = po.normalize(w_un)
        out["L"] = L
        out["max_idx"] = int(np.argmax(self.w))
        i = out["max_idx"]
        out["max_val"] = float(self.w[i])
        out["x_est"] = np.array([self.x[i], self.y[i], self.th[i]], dtype=np.float64)
        out["cov"] = np.asarray(po.weighted_cov(self.x.astype(np.float64), self.y.astype(np.float64),
                                                self.th.astype(np.float64),
                                                self.w.astype(np.float64)))
        out["ess"] = po.ess_of(self.w)
        out["resample_next"] = bool(out["ess"] < self.ess_th)
        return out

    def step(self, control, obs, noise, ofs=None):
        out = {"resampled": bool(self.needs_resample())}
        if out["resampled"]:
            self._resample(ofs, out)
        self._predict(control, noise)
        L, out["assoc"], out["margin"] = self.associate_update(obs)
        return self._step_end(L, out)


def update_loop(ref, obs):
    """``FSDARef.associate_update`` as a plain per-particle loop in matrix form
    (float64): returns (L, assoc) and updates ``ref`` in place."""
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 3)
    L = np.zeros(ref.n)
    assoc = np.empty((obs.shape[0], ref.n), dtype=np.int32)
    vo = ref.r_dir ** 2 + ref.r_orient ** 2
    for p in range(ref.n):
        pose = (ref.x[p], ref.y[p], ref.th[p])
        psi_p = np.pi / 2 - ref.th[p]
        c, s = np.cos(psi_p), np.sin(psi_p)
        cnt0 = int(ref.cnt[p])
        used = set()
        for q, (d, phi, psi) in enumerate(obs):
            R = np.diag(fr.scan_r(d, ref.r_dist, ref.r_dir))
            if ref.use_orient:
                e = float(fr.wrap(np.array(psi - float(fr.wrap(np.array(psi_p))))))
                L[p] -= e * e / (2 * vo)
            best, lbest, upd = -1, -np.inf, None
            for j in range(cnt0):
                if j in used:
                    continue
                P = np.array([[ref.cov[p, j, 0], ref.cov[p, j, 1]], [ref.cov[p, j, 1], ref.cov[p, j, 2]]])
                m, Pn, dl = fr.update_landmark_generic(pose, ref.mean[p, j].copy(), P, (d, phi), R)
                l = dl - np.log(2 * np.pi)
                if l > lbest:
                    best, lbest, upd = j, l, (m, Pn)
            if best < 0 or lbest < ref.log_p_new:
                L[p] += ref.log_p_new
                if ref.cnt[p] < ref.cap:
                    i = fr.init_landmark(ref.x[p], ref.y[p], c, s, d, phi, R[0, 0], R[1, 1])
                    j = int(ref.cnt[p])
                    ref.mean[p, j] = i[0], i[1]
                    ref.cov[p, j] = i[2], i[3], i[4]
                    ref.cnt[p] += 1
                    assoc[q, p] = NEW
                else:
                    assoc[q, p] = DROPPED
            else:
                L[p] += lbest
                ref.mean[p, best] = upd[0]
                ref.cov[p, best] = upd[1][0, 0], upd[1][0, 1], upd[1][1, 1]
                used.add(best)
                assoc[q, p] = best
    return L, assoc
