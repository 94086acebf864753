"""Long-double restatement of the EKF-SLAM update -- the test oracle of
slam_ekfslam_update at the 1e-11 level (tests/test_gpu_ekfslam_widths.py).

``update`` restates the update half of ekf_oracle.ekfslam_step
(oracle/ekf_oracle.py:186-263: measurement prediction, Jacobians, wrapped
innovations, scan_cov, K = P H^T S^-1, mu + K e, P - K (P H^T)^T) in
np.longdouble, with S inverted by a Gauss-Jordan elimination with partial
pivoting written out here (np.linalg.inv does not take long double).  The
prediction stays the float64 oracle's ekfslam_predict (pinned to 1e-13 on the
device by test_gpu_ekf.py).  ``spread`` is the float64 oracle's own distance
from the restatement -- the figure the device bar is set from -- and
``min_block_change`` says how far the update moves the least-moved 16 x 16
block of P, so that a skipped or stale block cannot hide under the bar.
Test infrastructure only: the shipped path never imports it.
"""
from __future__ import annotations

import functools

import numpy as np

import ekf_oracle as eo

LD = np.longdouble
DT = 0.1
Q_ROBOT = np.diag([0.1, 0.1, np.deg2rad(0.1)]) ** 2
NOISE = (0.05, np.deg2rad(2.0), np.deg2rad(2.0))
CTL = (1.0, 0.1)

# the fp64 constants the oracle (and the device) use, exactly, in long double
_PI = LD(np.pi)
_HALF_PI = LD(eo.HALF_PI)


def slam_world(n_lm, seed):
    """Landmarks, a prior mean near them and a dense positive-definite prior
    covariance (every landmark correlated with every other and with the robot)."""
    rs = np.random.RandomState(seed)
    lm = np.column_stack([rs.uniform(-30, 30, (n_lm, 2)), rs.uniform(-np.pi, np.pi, n_lm)])
    mu = np.concatenate([[0.0, 0.0, 0.3], (lm + rs.normal(0, 0.2, lm.shape)).ravel()])
    n = mu.size
    A = rs.normal(0, 0.02, (n, n // 3 + 1))
    P = A @ A.T + np.diag(np.concatenate([[0.01, 0.01, 0.002], np.full(n - 3, 0.04)]))
    P = 0.5 * (P + P.T)
    return rs, lm, mu, P


def wrap(a):
    """mylib/limit.py:11-26 for one long-double value."""
    r = abs(a)
    while r > _PI:
        r -= _PI * 2
    return -r if a < 0 else r


def inv_gauss_jordan(S):
    """Inverse of a square long-double matrix: Gauss-Jordan on [S | I] with
    partial (row) pivoting."""
    m = S.shape[0]
    A = np.concatenate([np.array(S, dtype=LD), np.eye(m, dtype=LD)], axis=1)
    for p in range(m):
        piv = p + int(np.argmax(np.abs(A[p:, p])))
        if piv != p:
            A[[p, piv]] = A[[piv, p]]
        A[p] = A[p] / A[p, p]
        col = A[:, p].copy()
        col[p] = 0
        A -= np.outer(col, A[p])
    return A[:, m:]


def measurement(mu, ids, obs, noise):
    """H restricted to its non-zero columns (m x (3 + 3k): the robot's three and
    each observation's own landmark block, as ekfslam_update_rows lays them
    out), the wrapped innovations, diag(R) and the state indices of those
    columns -- all in long double."""
    mu = np.asarray(mu, dtype=np.float64).astype(LD)
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 3).astype(LD)
    r_dist, r_dir, r_orient = (LD(v) for v in noise)
    k = len(ids)
    idx = [0, 1, 2]
    Hs = np.zeros((3 * k, 3 + 3 * k), dtype=LD)
    e = np.zeros(3 * k, dtype=LD)
    rd = np.zeros(3 * k, dtype=LD)
    x, y, th = mu[0], mu[1], mu[2]
    psi = _HALF_PI - th
    c, s = np.cos(psi), np.sin(psi)
    for t, j in enumerate(ids):
        j = int(j)
        idx += [3 + 3 * j, 4 + 3 * j, 5 + 3 * j]
        lx, ly, lp = mu[3 + 3 * j], mu[4 + 3 * j], mu[5 + 3 * j]
        dx, dy = lx - x, ly - y
        rx, ry = c * dx - s * dy, s * dx + c * dy
        zhat = (np.hypot(rx, ry), np.arctan2(ry, rx), wrap(psi + lp))
        q = dx * dx + dy * dy
        r = np.sqrt(q)
        Hs[3 * t:3 * t + 3, :3] = [[-dx / r, -dy / r, 0], [dy / q, -dx / q, -1], [0, 0, -1]]
        Hs[3 * t:3 * t + 3, 3 + 3 * t:6 + 3 * t] = [[dx / r, dy / r, 0], [-dy / q, dx / q, 0],
                                                    [0, 0, 1]]
        e[3 * t] = obs[t, 0] - zhat[0]
        e[3 * t + 1] = wrap(obs[t, 1] - zhat[1])
        e[3 * t + 2] = wrap(obs[t, 2] - zhat[2])
        rd[3 * t] = (obs[t, 0] * r_dist) ** 2
        rd[3 * t + 1] = (obs[t, 0] * np.sin(r_dir)) ** 2
        rd[3 * t + 2] = r_dir ** 2 + r_orient ** 2
    return Hs, e, rd, np.asarray(idx)


def update(mu, P, ids, obs, noise, aux=None):
    """The EKF-SLAM update from the predicted state (mu, P), in long double.
    Returns (mu + K e with the yaw wrapped, P - K (P H^T)^T), both long double;
    P's lower triangle is computed and mirrored (what the device stores).
    ``aux`` (a dict) receives S and the yaw before wrapping."""
    Hs, e, rd, idx = measurement(mu, ids, obs, noise)
    n = len(mu)
    Pl = np.asarray(P, dtype=np.float64)
    PHt = Pl[:, idx].astype(LD) @ Hs.T                  # n x m
    S = Hs @ PHt[idx] + np.diag(rd)
    K = PHt @ inv_gauss_jordan(S)
    mu_n = np.asarray(mu, dtype=np.float64).astype(LD) + K @ e
    if aux is not None:
        aux["S"] = S
        aux["yaw_unwrapped"] = mu_n[2]
    mu_n[2] = wrap(mu_n[2])
    Pn = np.empty((n, n), dtype=LD)
    step = 256
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        Pn[r0:r1, :r1] = Pl[r0:r1, :r1].astype(LD) - K[r0:r1] @ PHt[:r1].T
    iu = np.triu_indices(n, 1)
    Pn[iu] = Pn.T[iu]
    return mu_n, Pn


# ---------------------------------------------------------------- test cases
def make_ids(rs, n_lm, k, *, repeat=False):
    """k landmark ids, unsorted, with landmarks 0 and n_lm - 1 among them
    wherever k allows; ``repeat``: the first id named twice."""
    ids = rs.choice(n_lm, k, replace=False)
    if k >= 2 and n_lm >= 2:
        rest = [j for j in ids if j not in (0, n_lm - 1)][:k - 2]
        ids = np.array(rest[:len(rest) // 2] + [n_lm - 1] + rest[len(rest) // 2:] + [0])
    elif 0 not in ids:
        ids[0] = 0 if rs.rand() < 0.5 else n_lm - 1
    if repeat:
        ids[-1] = ids[0]
    return ids.astype(np.int64)


def make_obs(rs, xr, lm, ids):
    """ScanSensor triples of landmarks ``ids`` from the true pose xr, with noise."""
    k = len(ids)
    obs = np.array([eo.scan_predict(xr, lm[j]) for j in ids])
    obs[:, 0] *= 1 + rs.normal(0, 0.01, k)
    obs[:, 1:] += rs.normal(0, 0.01, (k, 2))
    return obs


class Case:
    """One update: the prior (mu0, P0), the control, the float64 oracle's
    predicted state (mu_p, P_p: what the device starts the update from) and the
    observation.  The references are computed on first use and kept."""

    def __init__(self, mu0, P0, ids, obs, ctl=CTL):
        self.mu0, self.P0, self.ctl = mu0, P0, ctl
        self.ids, self.obs = np.asarray(ids, dtype=np.int64), np.asarray(obs, dtype=np.float64)
        self.mu_p, self.P_p = eo.ekfslam_predict(mu0, P0, ctl, DT, Q_ROBOT)
        self.scale = float(np.abs(self.P_p).max())
        self.aux = {}

    @functools.cached_property
    def ld(self):
        return update(self.mu_p, self.P_p, self.ids, self.obs, NOISE, self.aux)

    @functools.cached_property
    def f64(self):
        mu, P = eo.ekfslam_step(self.mu0, self.P0, self.ctl, self.ids, self.obs, DT, Q_ROBOT, NOISE)
        return mu, 0.5 * (P + P.T)


def world_case(n_lm, k, seed=None, *, repeat=False, yaw=None, true_yaw=None):
    """A case on slam_world's prior.  ``yaw``: the predicted yaw wanted (the
    prior's is set so that the prediction lands there); ``true_yaw``: the yaw
    of the pose the observations are taken from."""
    rs, lm, mu, P = slam_world(n_lm, 1000 * n_lm + k if seed is None else seed)
    if yaw is not None:
        mu[2] = yaw - CTL[1] * DT
    xr = eo.ekf_motion(mu[:3], DT, *CTL)
    if true_yaw is not None:
        xr[2] = true_yaw
    ids = make_ids(rs, n_lm, k, repeat=repeat)
    return Case(mu, P, ids, make_obs(rs, xr, lm, ids))


@functools.lru_cache(maxsize=None)
def cached_case(n_lm, k, repeat=False):
    """The shared small cases (n <= 384): one reference for every test that names them."""
    return world_case(n_lm, k, repeat=repeat)


def spread(case):
    """(max |P64 - P_LD| / max |P_prior|, max |mu64 - mu_LD|): the float64
    oracle's ekfslam_step against the restatement, same predicted state."""
    if "spread" not in case.aux:
        mu_l, P_l = case.ld
        mu_d, P_d = case.f64
        case.aux["spread"] = (float(np.abs(P_d - P_l).max()) / case.scale,
                              float(np.abs(mu_d - mu_l).max()))
    return case.aux["spread"]


def slim(case):
    """Drop what a large case no longer needs once its spread is known (the
    prior and the float64 result); the predicted state and the restatement stay."""
    spread(case)
    case.P0 = None
    case.__dict__.pop("f64", None)
    return case


def min_block_change(case):
    """Smallest, over the 16 x 16 blocks of the lower triangle, of
    max |P_LD - P_prior| / max |P_prior|."""
    D = np.abs((case.ld[1] - case.P_p).astype(np.float64))
    n = D.shape[0]
    nb = (n + 15) // 16
    Dp = np.zeros((nb * 16, nb * 16))
    Dp[:n, :n] = D
    blk = Dp.reshape(nb, 16, nb, 16).max(axis=(1, 3))
    return float(blk[np.tril_indices(nb)].min()) / case.scale


def bars(case):
    """The device bars (P relative to max |P_prior|, mu absolute):
    max(1e-11, 64 x spread) -- test_gpu_fastslam.py's rule and floor."""
    sp = spread(case)
    return max(1e-11, 64 * sp[0]), max(1e-11, 64 * sp[1])


def errors(case, mu_dev, P_dev):
    """The device's distance from the restatement, in the units of ``bars``."""
    mu_l, P_l = case.ld
    return (float(np.abs(P_dev - P_l).max()) / case.scale, float(np.abs(mu_dev - mu_l).max()))


# the case tables of tests/test_gpu_ekfslam_widths.py (checked on the CPU by
# tests/test_ekfslam_ref.py)
ALL_WIDTHS = [(42, k) for k in range(1, 41)]
EDGE_SIZES = [1, 4, 5, 15, 85, 127]                      # n = 6, 15, 18, 48, 258, 384
EDGES = [(n_lm, k) for n_lm in EDGE_SIZES for k in (1, 5, 21, 22, 40) if k <= n_lm]
SEQUENCE_N_LM = 127
SEQUENCE = [40, 1, 21, 22, 3, 16]


def sequence_observation(step, k):
    """ids and obs of step ``step`` of the variable-width sequence: taken from
    the world's landmarks at the truth pose after step + 1 motions."""
    rs, lm, mu, _ = slam_world(SEQUENCE_N_LM, 77)
    rs = np.random.RandomState(7700 + step)
    xr = mu[:3].copy()
    for _ in range(step + 1):
        xr = eo.ekf_motion(xr, DT, *CTL)
    ids = make_ids(rs, SEQUENCE_N_LM, k)
    return ids, make_obs(rs, xr, lm, ids)


def multi_tile_n_lm(grid):
    """(nt, n_lm) of the smallest state whose tile count exceeds a resident
    grid: n = 128 (nt - 1) + 3 or so, one to three rows into the last tile row."""
    nt = 1
    while nt * (nt + 1) // 2 <= grid:
        nt += 1
    return nt, (128 * (nt - 1) + 3) // 3
