"""NumPy restatement of FastSLAM 2.0 without ids: per-particle maximum-likelihood
data association under the observation-informed proposal -- the test oracle of
slam_fs_create_assoc_proposal (include/slam_hip.h states the same contract).

The expressions are fastslam2_ref.FS2Ref.propose's (the three-state filter on
the pose) and fastslam_da_ref.FSDARef's (candidates, strict comparison, margins,
counts), put together: a candidate's score is the 2.0 seen-landmark likelihood,
linearised at the current proposal mean, with the pose covariance folded into
S.  ``FS2DARef`` is vectorised over particles and slots for a dtype parameter
(float64, and np.longdouble to measure float64's own rounding); ``step_loop``
is the same step as a plain per-particle Python loop in matrix form, which the
vectorised form is checked against.  Test infrastructure only: the shipped
path never imports it.
"""
from __future__ import annotations

import numpy as np

import fastslam2_ref as f2
import fastslam_da_ref as da
import fastslam_ref as fr
import pf_oracle as po

NEW, DROPPED = da.NEW, da.DROPPED


def score_terms(mux, muy, c, s, sig, mx, my, pxx, pxy, pyy, d, phi, R0, R1):
    """The seen-landmark step of FS2Ref.propose up to the score: returns
    (l without the -ln 2 pi, A (six arrays), S (three), det, e (two)).  Every
    argument broadcasts; ``sig`` is the six entries 00 01 02 11 12 22."""
    c00, c01, c02, c11, c12, c22 = sig
    dx, dy = mx - mux, my - muy
    q = dx * dx + dy * dy
    r = np.sqrt(q)
    bearing = np.arctan2(s * dx + c * dy, c * dx - s * dy)
    h00, h01, h10, h11 = dx / r, dy / r, -dy / q, dx / q
    t00, t01 = pxx * h00 + pxy * h01, pxx * h10 + pxy * h11
    t10, t11 = pxy * h00 + pyy * h01, pxy * h10 + pyy * h11
    a00, a01 = -(c00 * h00 + c01 * h01), -(c00 * h10 + c01 * h11) - c02
    a10, a11 = -(c01 * h00 + c11 * h01), -(c01 * h10 + c11 * h11) - c12
    a20, a21 = -(c02 * h00 + c12 * h01), -(c02 * h10 + c12 * h11) - c22
    s00 = (h00 * t00 + h01 * t10 + R0) - (h00 * a00 + h01 * a10)
    s01 = (h00 * t01 + h01 * t11) - (h00 * a01 + h01 * a11)
    s11 = (h10 * t01 + h11 * t11 + R1) - (h10 * a01 + h11 * a11 + a21)
    det = s00 * s11 - s01 * s01
    e0, e1 = d - r, fr.wrap(phi - bearing)
    maha = (e0 * e0 * s11 - 2 * (e0 * e1) * s01 + e1 * e1 * s00) / det
    return (-(maha + np.log(det)) / 2, (a00, a01, a10, a11, a20, a21), (s00, s01, s11), det,
            (e0, e1))


class FS2DARef(da.FSDARef):
    """FSDARef's state with the 2.0 step: ``step(control, obs, xi, ofs)`` takes
    three standard normals per particle and returns the usual outputs with the
    proposal (``mu``, ``sigma``, ``L``), the choices (``assoc`` [k][n]), every
    decision's margin and the smallest Cholesky pivots."""

    def __init__(self, n, cap, Q, **kw):
        assert kw.pop("motion", "linear") == "linear", "the 2.0 proposal is linear motion only"
        super().__init__(n, cap, motion="linear", **kw)
        self.Q = np.asarray(Q, dtype=np.float64)

    def propose(self, control, obs):
        """Step 2 of the contract from the current poses, counts and maps (which
        it only reads): (mu (3 arrays), Sigma (6 arrays), L, assoc, margin)."""
        t, n = self.t, self.n
        obs = np.asarray(obs, dtype=np.float64).reshape(-1, 3)
        k = obs.shape[0]
        v, om = control
        mux, muy, mut = po.motion_linear(self.x, self.y, self.th, self.dt, v, om)
        mux, muy, mut = mux.astype(t), muy.astype(t), mut.astype(t)
        Q = self.Q.astype(t)
        c00, c01, c02, c11, c12, c22 = (np.full(n, Q[i, j], dtype=t)
                                        for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))
        L = np.zeros(n, dtype=t)
        vo = t(self.r_dir) ** 2 + t(self.r_orient) ** 2
        lpn = t(self.log_p_new)
        ln2pi = np.log(2 * t(np.pi))
        cnt0 = self.cnt
        run = cnt0.copy()                               # the running count c
        jm = int(cnt0.max()) if n else 0
        matched = np.zeros((n, jm), dtype=bool)
        below = np.arange(jm)[None, :] < cnt0[:, None]
        rows = np.arange(n)
        assoc = np.empty((k, n), dtype=np.int32)
        margin = np.full((k, n), np.inf)
        mean, cov = self.mean[:, :jm], self.cov[:, :jm]
        for qi, z in enumerate(obs):
            d, phi, psi = (t(v_) for v_ in z)
            if self.use_orient:
                e = fr.wrap(psi - fr.wrap(t(np.pi / 2) - mut))
                so = c22 + vo
                L = L - (e * e / so + np.log(so)) / 2
                k0, k1, k2 = c02 / so, c12 / so, c22 / so
                b0, b1, b2 = c02, c12, c22
                mux, muy, mut = mux - k0 * e, muy - k1 * e, mut - k2 * e
                c00, c01, c02 = c00 - k0 * b0, c01 - k0 * b1, c02 - k0 * b2
                c11, c12, c22 = c11 - k1 * b1, c12 - k1 * b2, c22 - k2 * b2
            R0, R1 = fr.scan_r(d, t(self.r_dist), t(self.r_dir))
            allowed = below & ~matched
            has = allowed.any(axis=1)
            best = np.zeros(n, dtype=np.int64)
            lbest = np.full(n, -np.inf, dtype=t)
            if jm:
                psi_p = t(np.pi / 2) - mut
                c, s = np.cos(psi_p), np.sin(psi_p)
                col = lambda a: a[:, None]              # noqa: E731
                with np.errstate(all="ignore"):
                    l0, A, S, det, ee = score_terms(
                        col(mux), col(muy), col(c), col(s),
                        tuple(col(a) for a in (c00, c01, c02, c11, c12, c22)), mean[..., 0],
                        mean[..., 1], cov[..., 0], cov[..., 1], cov[..., 2], d, phi, R0, R1)
                    lj = l0 - ln2pi
                lj = np.where(allowed & ~np.isnan(lj), lj, -np.inf)
                best = np.argmax(lj, axis=1)            # the first of equal maxima: the lowest slot
                lbest = lj[rows, best]
                l2 = lj.copy()
                l2[rows, best] = -np.inf
                with np.errstate(invalid="ignore"):
                    mg = np.abs(lbest - lpn)
                    mg = np.where(lbest < lpn, mg, np.minimum(mg, lbest - l2.max(axis=1)))
                margin[qi, has] = mg[has].astype(np.float64)
            match = has & ~(lbest < lpn)
            new = ~match
            room = new & (run < self.cap)
            assoc[qi] = np.where(match, best, np.where(room, NEW, DROPPED))
            run = run + room
            L = np.where(new, L + lpn, L)
            pm = np.flatnonzero(match)
            if pm.size:
                bm = best[pm]
                pick = lambda a: a[pm, bm]              # noqa: E731
                a00, a01, a10, a11, a20, a21 = (pick(a) for a in A)
                s00, s01, s11 = (pick(a) for a in S)
                dt_, e0, e1 = pick(det), pick(ee[0]), pick(ee[1])
                L[pm] = L[pm] + lbest[pm]
                k00, k01 = (a00 * s11 - a01 * s01) / dt_, (a01 * s00 - a00 * s01) / dt_
                k10, k11 = (a10 * s11 - a11 * s01) / dt_, (a11 * s00 - a10 * s01) / dt_
                k20, k21 = (a20 * s11 - a21 * s01) / dt_, (a21 * s00 - a20 * s01) / dt_
                mux, muy, mut = mux.copy(), muy.copy(), mut.copy()
                c00, c01, c02, c11, c12, c22 = (a.copy() for a in (c00, c01, c02, c11, c12, c22))
                mux[pm] = mux[pm] + (k00 * e0 + k01 * e1)
                muy[pm] = muy[pm] + (k10 * e0 + k11 * e1)
                mut[pm] = mut[pm] + (k20 * e0 + k21 * e1)
                c00[pm] = c00[pm] - (k00 * a00 + k01 * a01)
                c01[pm] = c01[pm] - (k00 * a10 + k01 * a11)
                c02[pm] = c02[pm] - (k00 * a20 + k01 * a21)
                c11[pm] = c11[pm] - (k10 * a10 + k11 * a11)
                c12[pm] = c12[pm] - (k10 * a20 + k11 * a21)
                c22[pm] = c22[pm] - (k20 * a20 + k21 * a21)
                matched[pm, bm] = True
        return (mux, muy, mut), (c00, c01, c02, c11, c12, c22), L, assoc, margin

    def update_maps(self, obs, assoc):
        """Step 4: the maps at the current (sampled) poses by the recorded choices."""
        t = self.t
        psi_p = t(np.pi / 2) - self.th
        c, s = np.cos(psi_p), np.sin(psi_p)
        for z, a in zip(np.asarray(obs, dtype=np.float64).reshape(-1, 3), assoc):
            d, phi, _ = (t(v_) for v_ in z)
            R0, R1 = fr.scan_r(d, t(self.r_dist), t(self.r_dir))
            pm = np.flatnonzero(a >= 0)
            if pm.size:
                bm = a[pm]
                r = fr.update_landmark(self.x[pm], self.y[pm], c[pm], s[pm], self.mean[pm, bm, 0],
                                       self.mean[pm, bm, 1], self.cov[pm, bm, 0], self.cov[pm, bm, 1],
                                       self.cov[pm, bm, 2], d, phi, R0, R1)
                self.mean[pm, bm, 0], self.mean[pm, bm, 1] = r[0], r[1]
                self.cov[pm, bm, 0], self.cov[pm, bm, 1], self.cov[pm, bm, 2] = r[2], r[3], r[4]
            pr = np.flatnonzero(a == NEW)
            if pr.size:
                i = fr.init_landmark(self.x[pr], self.y[pr], c[pr], s[pr], d, phi, R0, R1)
                sl = self.cnt[pr]
                self.mean[pr, sl, 0], self.mean[pr, sl, 1] = i[0], i[1]
                self.cov[pr, sl, 0], self.cov[pr, sl, 1], self.cov[pr, sl, 2] = i[2], i[3], i[4]
                self.cnt[pr] += 1

    def step(self, control, obs, xi, ofs=None):
        t = self.t
        out = {"resampled": bool(self.needs_resample())}
        if out["resampled"]:
            self._resample(ofs, out)
        (mux, muy, mut), sig, L, out["assoc"], out["margin"] = self.propose(control, obs)
        (l00, l10, l20, l11, l21, l22), piv = f2.chol3(*sig)
        out["pivots"] = tuple(float(np.min(v)) for v in piv)
        assert all(np.all(v > 0) for v in piv), f"non-positive Cholesky pivot: {out['pivots']}"
        xi = np.asarray(xi).astype(t)
        self.x = mux + l00 * xi[:, 0]
        self.y = muy + (l10 * xi[:, 0] + l11 * xi[:, 1])
        self.th = mut + (l20 * xi[:, 0] + l21 * xi[:, 1] + l22 * xi[:, 2])
        out["mu"] = np.column_stack([mux, muy, mut])
        out["sigma"] = np.column_stack(sig)
        self.update_maps(obs, out["assoc"])
        return self._step_end(L, out)


def step_loop(ref, control, obs, xi):
    """``FS2DARef``'s steps 2 to 4 as a plain per-particle loop in matrix form
    (float64; np.linalg for S^-1, K = Sigma H_x^T S^-1, Sigma - K H_x Sigma, the
    Cholesky factor): returns (mu [n][3], Sigma [n][3][3], L, assoc) and updates
    poses, counts and maps of ``ref`` in place."""
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 3)
    n, k = ref.n, obs.shape[0]
    v, om = control
    vo = ref.r_dir ** 2 + ref.r_orient ** 2
    mus, sigmas, L = np.empty((n, 3)), np.empty((n, 3, 3)), np.zeros(n)
    assoc = np.empty((k, n), dtype=np.int32)
    for p in range(n):
        mu = np.array([float(a[0]) for a in po.motion_linear(ref.x[p:p + 1], ref.y[p:p + 1],
                                                            ref.th[p:p + 1], ref.dt, v, om)])
        Sig = ref.Q.copy()
        cnt0, run, used = int(ref.cnt[p]), int(ref.cnt[p]), set()
        for qi, (d, phi, psi) in enumerate(obs):
            R = np.diag(fr.scan_r(d, ref.r_dist, ref.r_dir))
            if ref.use_orient:
                H = np.array([[0.0, 0.0, -1.0]])
                e = float(fr.wrap(np.array(psi - float(fr.wrap(np.array(np.pi / 2 - mu[2]))))))
                so = (H @ Sig @ H.T)[0, 0] + vo
                L[p] -= (e * e / so + np.log(so)) / 2
                K = Sig @ H.T / so
                mu = mu + K[:, 0] * e
                Sig = Sig - K @ H @ Sig
            c, s = np.cos(np.pi / 2 - mu[2]), np.sin(np.pi / 2 - mu[2])
            best, lbest, upd = -1, -np.inf, None
            for j in range(cnt0):
                if j in used:
                    continue
                dx, dy = ref.mean[p, j] - mu[:2]
                q = dx * dx + dy * dy
                r = np.sqrt(q)
                Hm = np.array([[dx / r, dy / r], [-dy / q, dx / q]])
                Hx = np.hstack([-Hm, [[0.0], [-1.0]]])
                P = np.array([[ref.cov[p, j, 0], ref.cov[p, j, 1]], [ref.cov[p, j, 1], ref.cov[p, j, 2]]])
                e2 = np.array([d - r, float(fr.wrap(np.array(
                    phi - np.arctan2(s * dx + c * dy, c * dx - s * dy))))])
                S = Hm @ P @ Hm.T + R + Hx @ Sig @ Hx.T
                Si = np.linalg.inv(S)
                l = -(e2 @ Si @ e2 + np.log(np.linalg.det(S))) / 2 - np.log(2 * np.pi)
                if l > lbest:
                    best, lbest, upd = j, l, (Hx, Si, e2)
            if best < 0 or lbest < ref.log_p_new:
                L[p] += ref.log_p_new
                if run < ref.cap:
                    assoc[qi, p] = NEW
                    run += 1
                else:
                    assoc[qi, p] = DROPPED
            else:
                Hx, Si, e2 = upd
                L[p] += lbest
                K = Sig @ Hx.T @ Si
                mu = mu + K @ e2
                Sig = Sig - K @ Hx @ Sig
                used.add(best)
                assoc[qi, p] = best
        mus[p], sigmas[p] = mu, Sig
        pose = mu + np.linalg.cholesky(Sig) @ np.asarray(xi[p], dtype=np.float64)
        ref.x[p], ref.y[p], ref.th[p] = pose
        c, s = np.cos(np.pi / 2 - pose[2]), np.sin(np.pi / 2 - pose[2])
        for qi, (d, phi, _) in enumerate(obs):
            R = np.diag(fr.scan_r(d, ref.r_dist, ref.r_dir))
            a = int(assoc[qi, p])
            if a >= 0:
                P = np.array([[ref.cov[p, a, 0], ref.cov[p, a, 1]], [ref.cov[p, a, 1], ref.cov[p, a, 2]]])
                m, Pn, _ = fr.update_landmark_generic(tuple(pose), ref.mean[p, a].copy(), P, (d, phi), R)
                ref.mean[p, a] = m
                ref.cov[p, a] = Pn[0, 0], Pn[0, 1], Pn[1, 1]
            elif a == NEW:
                i = fr.init_landmark(pose[0], pose[1], c, s, d, phi, R[0, 0], R[1, 1])
                j = int(ref.cnt[p])
                ref.mean[p, j] = i[0], i[1]
                ref.cov[p, j] = i[2], i[3], i[4]
                ref.cnt[p] += 1
    return mus, sigmas, L, assoc
