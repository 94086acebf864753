"""NumPy restatement of FastSLAM 1.0 with known data association -- the test
oracle of slam_fs_* (include/slam_hip.h states the same contract).

Only what is new is written here, for a dtype parameter (float64, and
np.longdouble to measure float64's own rounding); the motion models,
``normalize``, ``ess_of``, ``systematic_indices`` and ``weighted_cov`` are
pf_oracle's.  Test infrastructure only: the shipped path never imports it.
"""
from __future__ import annotations

import numpy as np

import pf_oracle as po


def wrap(a):
    """mylib/limit.py:11-26 per element, in a's dtype."""
    a0 = np.asarray(a)
    a = np.atleast_1d(a0)
    r = np.absolute(a).copy()
    two_pi = a.dtype.type(np.pi) * 2
    m = r > np.pi
    while m.any():
        r[m] -= two_pi
        m = r > np.pi
    r[a < 0] *= -1
    return r.reshape(a0.shape)


def scan_r(d, r_dist, r_dir):
    """The range / bearing entries of ekf_oracle.scan_cov at the observed range."""
    return (d * r_dist) ** 2, (d * np.sin(r_dir)) ** 2


def init_landmark(x, y, c, s, d, phi, R0, R1):
    """First sighting: mean and covariance (pxx, pxy, pyy) per particle."""
    rx, ry = d * np.cos(phi), d * np.sin(phi)
    dx = c * rx + s * ry
    dy = -s * rx + c * ry
    q = dx * dx + dy * dy
    r = np.sqrt(q)
    a00, a01, a10, a11 = dx / r, -dy, dy / r, dx
    return (x + dx, y + dy, a00 * a00 * R0 + a01 * a01 * R1, a00 * a10 * R0 + a01 * a11 * R1,
            a10 * a10 * R0 + a11 * a11 * R1)


def update_landmark(x, y, c, s, mx, my, pxx, pxy, pyy, d, phi, R0, R1):
    """Scalar 2 x 2 EKF update of one seen landmark per particle.  Returns the
    new (mx, my, pxx, pxy, pyy) and the log-weight term."""
    dx, dy = mx - x, my - y
    q = dx * dx + dy * dy
    r = np.sqrt(q)
    bearing = np.arctan2(s * dx + c * dy, c * dx - s * dy)
    h00, h01, h10, h11 = dx / r, dy / r, -dy / q, dx / q
    t00, t01 = pxx * h00 + pxy * h01, pxx * h10 + pxy * h11
    t10, t11 = pxy * h00 + pyy * h01, pxy * h10 + pyy * h11
    s00 = h00 * t00 + h01 * t10 + R0
    s01 = h00 * t01 + h01 * t11
    s11 = h10 * t01 + h11 * t11 + R1
    det = s00 * s11 - s01 * s01
    e0, e1 = d - r, wrap(phi - bearing)
    maha = (e0 * e0 * s11 - 2 * (e0 * e1) * s01 + e1 * e1 * s00) / det
    dl = -(maha + np.log(det)) / 2
    k00, k01 = (t00 * s11 - t01 * s01) / det, (t01 * s00 - t00 * s01) / det
    k10, k11 = (t10 * s11 - t11 * s01) / det, (t11 * s00 - t10 * s01) / det
    m00, m01 = k00 * s00 + k01 * s01, k00 * s01 + k01 * s11
    m10, m11 = k10 * s00 + k11 * s01, k10 * s01 + k11 * s11
    return (mx + (k00 * e0 + k01 * e1), my + (k10 * e0 + k11 * e1),
            pxx - (m00 * k00 + m01 * k01), pxy - (m00 * k10 + m01 * k11),
            pyy - (m10 * k10 + m11 * k11), dl)


def update_landmark_generic(pose, mean, P, z, R):
    """The same update in matrix form (np.linalg.inv, K = P H^T S^-1,
    P - K S K^T) for one particle: what the scalar form is checked against."""
    x, y, th = pose
    c, s = np.cos(np.pi / 2 - th), np.sin(np.pi / 2 - th)
    dx, dy = mean[0] - x, mean[1] - y
    q = dx * dx + dy * dy
    r = np.sqrt(q)
    H = np.array([[dx / r, dy / r], [-dy / q, dx / q]])
    zhat = np.array([r, np.arctan2(s * dx + c * dy, c * dx - s * dy)])
    e = np.array([z[0] - zhat[0], float(wrap(np.array(z[1] - zhat[1])))])
    S = H @ P @ H.T + R
    Si = np.linalg.inv(S)
    K = P @ H.T @ Si
    dl = -(e @ Si @ e + np.log(np.linalg.det(S))) / 2
    return mean + K @ e, P - K @ S @ K.T, dl


class FSRef:
    """State and one step of the filter, in ``dtype``."""

    def __init__(self, n, nl, *, dt=0.1, motion="linear", alphas=(0.1,) * 6,
                 noise=(0.1, np.deg2rad(3.0), np.deg2rad(3.0)), use_orient=True, ess_th=None,
                 x0=(10.0, 0.0, np.pi / 2), dtype=np.float64):
        self.n, self.nl, self.dt, self.motion, self.alphas = n, nl, dt, motion, tuple(alphas)
        self.r_dist, self.r_dir, self.r_orient = noise
        self.use_orient = use_orient
        self.ess_th = n / 100.0 if ess_th is None else ess_th
        self.t = dtype
        self.x = np.full(n, x0[0], dtype=dtype)
        self.y = np.full(n, x0[1], dtype=dtype)
        self.th = np.full(n, x0[2], dtype=dtype)
        self.w = np.full(n, 1 / n, dtype=dtype)
        self.seen = np.zeros(nl, dtype=bool)
        self.mean = np.full((n, nl, 2), np.nan, dtype=dtype)
        self.cov = np.full((n, nl, 3), np.nan, dtype=dtype)

    def load(self, other):
        """Take another instance's state (cast to this dtype)."""
        for k in ("x", "y", "th", "w", "mean", "cov"):
            setattr(self, k, getattr(other, k).astype(self.t))
        self.seen = other.seen.copy()

    def needs_resample(self):
        return po.ess_of(self.w) < self.ess_th

    def step(self, control, ids, obs, noise, ofs=None):
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
        v, om = control
        noise = np.asarray(noise).astype(t)
        if self.motion == "linear":
            xn, yn, tn = po.motion_linear(self.x, self.y, self.th, self.dt, v, om)
            self.x, self.y, self.th = xn + noise[:, 0], yn + noise[:, 1], tn.astype(t) + noise[:, 2]
        else:
            xn, yn, tn = po.motion_velocity(self.x, self.y, self.th, v, om, self.dt, self.alphas,
                                            noise)
            self.x, self.y, self.th = xn, yn, tn.astype(t)
        psi_p = t(np.pi / 2) - self.th
        c, s = np.cos(psi_p), np.sin(psi_p)
        psi_w = wrap(psi_p)
        L = np.zeros(self.n, dtype=t)
        for j, z in zip(ids, np.asarray(obs, dtype=np.float64).reshape(-1, 3)):
            d, phi, psi = (t(v_) for v_ in z)
            R0, R1 = scan_r(d, t(self.r_dist), t(self.r_dir))
            if self.use_orient:
                e = wrap(psi - psi_w)
                L -= e * e / (2 * (t(self.r_dir) ** 2 + t(self.r_orient) ** 2))
            if not self.seen[j]:
                r = init_landmark(self.x, self.y, c, s, d, phi, R0, R1)
            else:
                r = update_landmark(self.x, self.y, c, s, self.mean[:, j, 0], self.mean[:, j, 1],
                                    self.cov[:, j, 0], self.cov[:, j, 1], self.cov[:, j, 2], d, phi,
                                    R0, R1)
                L += r[5]
            self.mean[:, j, 0], self.mean[:, j, 1] = r[0], r[1]
            self.cov[:, j, 0], self.cov[:, j, 1], self.cov[:, j, 2] = r[2], r[3], r[4]
        self.seen[np.asarray(ids, dtype=np.int64)] = True
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


# ------------------------------------------------------------- test worlds
def observe(pose, lm, rng_range, noise, rs):
    """ScanSensor's triples (range, bearing, orientation) of the landmarks
    within rng_range of the true pose, with its noise model; landmark headings
    are zero.  Returns (ids, obs)."""
    r_dist, r_dir, r_orient = noise
    psi = np.pi / 2 - pose[2]
    c, s = np.cos(psi), np.sin(psi)
    dx, dy = lm[:, 0] - pose[0], lm[:, 1] - pose[1]
    rx, ry = c * dx - s * dy, s * dx + c * dy
    d = np.hypot(rx, ry)
    ids = np.flatnonzero(d <= rng_range)
    g = rs.standard_normal((ids.size, 3))
    obs = np.column_stack([d[ids] * (1 + r_dist * g[:, 0]), np.arctan2(ry, rx)[ids] + r_dir * g[:, 1],
                           float(po.wrap_angle(psi)) + r_orient * g[:, 2]])
    return ids.astype(np.int64), obs


def circle_truth(steps, dt=0.1, x0=(10.0, 0.0, np.pi / 2)):
    """The reference's circle (particle_filter.py:46-48): control and true poses."""
    om = np.deg2rad(10.0)
    v = 10.0 * om
    pose = np.array(x0, dtype=np.float64)
    poses = []
    for _ in range(steps):
        pose = np.array(po.motion_velocity_exact(pose, v, om, dt))
        poses.append(pose)
    return (v, om), poses
