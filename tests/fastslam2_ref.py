"""NumPy restatement of the FastSLAM 2.0 step (slam_fs_create_proposal;
include/slam_hip.h states the same contract) on top of fastslam_ref: known
data association, linear motion, the pose drawn from the proposal that has
seen the step's scan.

Scalar form, vectorised over the particles, for a dtype parameter (float64,
and np.longdouble to measure float64's own rounding).  Test infrastructure
only: the shipped path never imports it.
"""
from __future__ import annotations

import numpy as np

import fastslam_ref as fr
import pf_oracle as po


def q_from_factor(F):
    """Q = F^T F as the handle forms it: Q[i][j] = sum_k F[k][i] F[k][j], k ascending."""
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    return np.array([[(F[0, i] * F[0, j] + F[1, i] * F[1, j]) + F[2, i] * F[2, j]
                      for j in range(3)] for i in range(3)])


def chol3(c00, c01, c02, c11, c12, c22):
    """Lower Cholesky factor of symmetric 3 x 3 matrices, entry by entry; the
    pivots (the arguments of the three square roots) beside it."""
    l00 = np.sqrt(c00)
    l10, l20 = c01 / l00, c02 / l00
    p1 = c11 - l10 * l10
    l11 = np.sqrt(p1)
    l21 = (c12 - l20 * l10) / l11
    p2 = c22 - l20 * l20 - l21 * l21
    l22 = np.sqrt(p2)
    return (l00, l10, l20, l11, l21, l22), (c00, p1, p2)


class FS2Ref(fr.FSRef):
    """FSRef with the FastSLAM 2.0 step: ``step(control, ids, obs, xi, ofs)``
    takes three standard normals per particle and returns the usual outputs
    with the proposal (``mu`` [n][3], ``sigma`` [n][6]: 00 01 02 11 12 22, ``L``)
    and the smallest Cholesky pivots (``pivots``)."""

    def __init__(self, n, nl, Q, **kw):
        assert kw.pop("motion", "linear") == "linear", "the 2.0 proposal is linear motion only"
        super().__init__(n, nl, motion="linear", **kw)
        self.Q = np.asarray(Q, dtype=np.float64)

    def propose(self, control, ids, obs):
        """mu (3 arrays), Sigma (6 arrays) and L of every particle for one scan,
        from the current poses and maps."""
        t = self.t
        v, om = control
        mux, muy, mut = po.motion_linear(self.x, self.y, self.th, self.dt, v, om)
        mux, muy, mut = mux.astype(t), muy.astype(t), mut.astype(t)
        Q = self.Q.astype(t)
        c00, c01, c02, c11, c12, c22 = (np.full(self.n, Q[i, j], dtype=t)
                                        for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))
        L = np.zeros(self.n, dtype=t)
        vo = t(self.r_dir) ** 2 + t(self.r_orient) ** 2
        for j, z in zip(ids, np.asarray(obs, dtype=np.float64).reshape(-1, 3)):
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
            if not self.seen[j]:
                continue
            R0, R1 = fr.scan_r(d, t(self.r_dist), t(self.r_dir))
            mx, my = self.mean[:, j, 0], self.mean[:, j, 1]
            pxx, pxy, pyy = self.cov[:, j, 0], self.cov[:, j, 1], self.cov[:, j, 2]
            psi_p = t(np.pi / 2) - mut
            c, s = np.cos(psi_p), np.sin(psi_p)
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
            L = L - (maha + np.log(det)) / 2
            k00, k01 = (a00 * s11 - a01 * s01) / det, (a01 * s00 - a00 * s01) / det
            k10, k11 = (a10 * s11 - a11 * s01) / det, (a11 * s00 - a10 * s01) / det
            k20, k21 = (a20 * s11 - a21 * s01) / det, (a21 * s00 - a20 * s01) / det
            mux, muy, mut = (mux + (k00 * e0 + k01 * e1), muy + (k10 * e0 + k11 * e1),
                             mut + (k20 * e0 + k21 * e1))
            c00, c01, c02 = (c00 - (k00 * a00 + k01 * a01), c01 - (k00 * a10 + k01 * a11),
                             c02 - (k00 * a20 + k01 * a21))
            c11, c12 = c11 - (k10 * a10 + k11 * a11), c12 - (k10 * a20 + k11 * a21)
            c22 = c22 - (k20 * a20 + k21 * a21)
        return (mux, muy, mut), (c00, c01, c02, c11, c12, c22), L

    def step(self, control, ids, obs, xi, ofs=None):
        t = self.t
        out = {"resampled": bool(self.needs_resample())}
        if out["resampled"]:
            idx = po.systematic_indices(self.w, t(ofs))
            if (idx < 0).any():
                raise IndexError("resample position beyond the last cumulative weight")
            out["idx"] = idx
            self.x, self.y, self.th = self.x[idx], self.y[idx], self.th[idx]
            self.mean, self.cov = self.mean[idx], self.cov[idx]
            self.w = np.full(self.n, 1 / self.n, dtype=t)
        ids = np.asarray(ids, dtype=np.int64)
        (mux, muy, mut), sig, L = self.propose(control, ids, obs)
        (l00, l10, l20, l11, l21, l22), piv = chol3(*sig)
        out["pivots"] = tuple(float(np.min(v)) for v in piv)
        assert all(np.all(v > 0) for v in piv), f"non-positive Cholesky pivot: {out['pivots']}"
        xi = np.asarray(xi).astype(t)
        self.x = mux + l00 * xi[:, 0]
        self.y = muy + (l10 * xi[:, 0] + l11 * xi[:, 1])
        self.th = mut + (l20 * xi[:, 0] + l21 * xi[:, 1] + l22 * xi[:, 2])
        out["mu"] = np.column_stack([mux, muy, mut])
        out["sigma"] = np.column_stack(sig)
        # the maps at the sampled pose: the 1.0 update without its weight term
        psi_p = t(np.pi / 2) - self.th
        c, s = np.cos(psi_p), np.sin(psi_p)
        for j, z in zip(ids, np.asarray(obs, dtype=np.float64).reshape(-1, 3)):
            d, phi, _ = (t(v_) for v_ in z)
            R0, R1 = fr.scan_r(d, t(self.r_dist), t(self.r_dir))
            if not self.seen[j]:
                r = fr.init_landmark(self.x, self.y, c, s, d, phi, R0, R1)
            else:
                r = fr.update_landmark(self.x, self.y, c, s, self.mean[:, j, 0], self.mean[:, j, 1],
                                       self.cov[:, j, 0], self.cov[:, j, 1], self.cov[:, j, 2], d,
                                       phi, R0, R1)
            self.mean[:, j, 0], self.mean[:, j, 1] = r[0], r[1]
            self.cov[:, j, 0], self.cov[:, j, 1], self.cov[:, j, 2] = r[2], r[3], r[4]
        self.seen[ids] = True
        w_un = self.w * np.exp(L - np.max(L))
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
