"""NumPy restatement of EKF-SLAM without ids -- the test oracle of an
associating slam_ekfslam handle (include/slam_hip.h states the same contract):
maximum-likelihood association against every landmark held, each landmark at
most once per scan, landmark initialisation below ``p_new``, a map that grows.

``scores`` is vectorised over the slots for a dtype parameter (float64, and
np.longdouble to measure float64's own rounding); ``scores_loop`` is the same
score as a plain per-slot loop on ekf_oracle's scan_predict / scan_jacobian /
scan_cov and np.linalg, which the vectorised form is checked against.  The
update of the matched observations is ekf_oracle's arithmetic in float64
(``update_f64``) and tests/ekfslam_ref.py's ``update`` in long double, both on
the active prefix.  ``choose`` also returns every decision's margin:
``|l_best - log_p_new|``, and ``l_best - l_second`` as well where the best
candidate is taken; infinite where there is no candidate.

A chain (``run``) carries its state in float64 between steps in either dtype,
and predicts with the float64 oracle (ekfslam_ref's convention): the dtype is
the arithmetic of one ``observe``.
Test infrastructure only: the shipped path never imports it.
"""
from __future__ import annotations

import functools

import numpy as np

import ekf_oracle as eo
import ekfslam_ref as er

NEW, DROPPED = -1, -2
LD = np.longdouble
MAX_OBS = 40
DT, Q_ROBOT, NOISE = er.DT, er.Q_ROBOT, er.NOISE


def wrap(a, t):
    """mylib/limit.py:11-26, elementwise in dtype t."""
    a = np.asarray(a, dtype=t)
    pi = t(np.pi)
    r = np.abs(a)
    while np.any(r > pi):
        r = np.where(r > pi, r - pi * 2, r)
    return np.where(a < 0, -r, r)


def scan_r(d, noise, t):
    """diag(scan_cov(d)) in dtype t."""
    r_dist, r_dir, r_orient = (t(v) for v in noise)
    return np.array([(d * r_dist) ** 2, (d * np.sin(r_dir)) ** 2, r_dir ** 2 + r_orient ** 2],
                    dtype=t)


# ------------------------------------------------------------------ scores
def scores(mu, P, count, obs, noise=NOISE, t=np.float64):
    """l[k][count]: log-likelihood of each observation under each slot, from
    the 6 x 6 block of P over the robot and the slot; determinant and quadratic
    form of the 3 x 3 S through its cofactors."""
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 3).astype(t)
    k = obs.shape[0]
    if count == 0:
        return np.empty((k, 0), dtype=t)
    na = 3 + 3 * count
    mu = np.asarray(mu)[:na].astype(t)
    Pa = np.asarray(P)[:na, :na]                         # only the 6 x 6 blocks are converted
    x, y, th = mu[:3]
    L = mu[3:].reshape(count, 3)
    psi = t(eo.HALF_PI) - th
    c, s = np.cos(psi), np.sin(psi)
    dx, dy = L[:, 0] - x, L[:, 1] - y
    rx, ry = c * dx - s * dy, s * dx + c * dy
    zh = np.stack([np.hypot(rx, ry), np.arctan2(ry, rx), wrap(psi + L[:, 2], t)], axis=1)
    q = dx * dx + dy * dy
    r = np.sqrt(q)
    H = np.zeros((count, 3, 6), dtype=t)
    H[:, 0, 0], H[:, 0, 1], H[:, 0, 3], H[:, 0, 4] = -dx / r, -dy / r, dx / r, dy / r
    H[:, 1, 0], H[:, 1, 1], H[:, 1, 2], H[:, 1, 3], H[:, 1, 4] = dy / q, -dx / q, -1, -dy / q, dx / q
    H[:, 2, 2], H[:, 2, 5] = -1, 1
    B = np.empty((count, 6, 6), dtype=t)
    B[:, :3, :3] = Pa[:3, :3]
    B[:, 3:, :3] = Pa[3:, :3].reshape(count, 3, 3)
    B[:, :3, 3:] = B[:, 3:, :3].transpose(0, 2, 1)
    idx = 3 + 3 * np.arange(count)[:, None] + np.arange(3)
    B[:, 3:, 3:] = Pa[idx[:, :, None], idx[:, None, :]]
    A = np.einsum("jau,juv,jbv->jab", H, B, H)
    out = np.empty((k, count), dtype=t)
    ln2pi = np.log(2 * t(np.pi))
    with np.errstate(all="ignore"):
        for i, z in enumerate(obs):
            R = scan_r(z[0], noise, t)
            e0 = z[0] - zh[:, 0]
            e1 = wrap(z[1] - zh[:, 1], t)
            e2 = wrap(z[2] - zh[:, 2], t)
            s00, s11, s22 = A[:, 0, 0] + R[0], A[:, 1, 1] + R[1], A[:, 2, 2] + R[2]
            s01, s02, s12 = A[:, 1, 0], A[:, 2, 0], A[:, 2, 1]
            c00 = s11 * s22 - s12 * s12
            c01 = s02 * s12 - s01 * s22
            c02 = s01 * s12 - s02 * s11
            c11 = s00 * s22 - s02 * s02
            c12 = s01 * s02 - s00 * s12
            c22 = s00 * s11 - s01 * s01
            det = (s00 * c00 + s01 * c01) + s02 * c02
            dg = (e0 * e0 * c00 + e1 * e1 * c11) + e2 * e2 * c22
            od = (e0 * e1 * c01 + e0 * e2 * c02) + e1 * e2 * c12
            out[i] = -(((dg + 2 * od) / det) + np.log(det)) / 2 - 3 * ln2pi / 2
    return out


def scores_loop(mu, P, count, obs, noise=NOISE):
    """``scores`` as a plain loop over observations and slots, in matrix form
    on the oracle's functions (float64)."""
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 3)
    out = np.empty((obs.shape[0], count))
    for i, z in enumerate(obs):
        R = eo.scan_cov(z[0], *noise)
        for j in range(count):
            idx = np.r_[0:3, 3 + 3 * j:6 + 3 * j]
            lm = mu[3 + 3 * j:6 + 3 * j]
            Hr, Hl = eo.scan_jacobian(mu[:3], lm)
            H = np.hstack([Hr, Hl])
            e = z - eo.scan_predict(mu[:3], lm)
            e[1], e[2] = eo.wrap_angle(e[1]), eo.wrap_angle(e[2])
            S = H @ P[np.ix_(idx, idx)] @ H.T + R
            out[i, j] = -(e @ np.linalg.solve(S, e) + np.log(np.linalg.det(S))) / 2 \
                - 1.5 * np.log(2 * np.pi)
    return out


# ------------------------------------------------------------------ choice
def choose(l, log_p_new, count0, cap):
    """The greedy choice over the score rows: (assoc [k], margin [k])."""
    k = l.shape[0]
    taken = np.zeros(count0, dtype=bool)
    count = count0
    assoc = np.empty(k, dtype=np.int32)
    margin = np.full(k, np.inf)
    lpn = l.dtype.type(log_p_new)
    for i in range(k):
        best, lb = -1, -np.inf
        if count0:
            row = np.where(~taken & ~np.isnan(l[i]), l[i], -np.inf)
            best = int(np.argmax(row))             # the first of equal maxima: the lowest slot
            lb = row[best]
            if lb == -np.inf:
                best = -1
        if best >= 0:
            mg = abs(lb - lpn)
            if not lb < lpn:
                row[best] = -np.inf
                mg = min(mg, lb - row.max())
            margin[i] = float(mg)
        if best < 0 or lb < lpn:
            if count < cap:
                assoc[i] = NEW
                count += 1
            else:
                assoc[i] = DROPPED
        else:
            assoc[i] = best
            taken[best] = True
    return assoc, margin


# ---------------------------------------------------------- initialisation
def inverse_model(xr, z, t=np.float64):
    """g(x, z): the landmark (x, y, phi) that scan_predict maps back to z, and
    the offset (dx, dy)."""
    x, y, th = (t(v) for v in xr)
    d, b, o = (t(v) for v in z)
    psi = t(eo.HALF_PI) - th
    c, s = np.cos(psi), np.sin(psi)
    rx, ry = d * np.cos(b), d * np.sin(b)
    dx, dy = c * rx + s * ry, -s * rx + c * ry
    return np.array([x + dx, y + dy, wrap(o - psi, t)], dtype=t), dx, dy


def init_jacobians(xr, z, t=np.float64):
    """G_r = dg/d(robot), G_z = dg/d(range, bearing, orientation)."""
    _, dx, dy = inverse_model(xr, z, t)
    d = t(z[0])
    Gr = np.array([[1, 0, -dy], [0, 1, dx], [0, 0, 1]], dtype=t)
    Gz = np.array([[dx / d, -dy, 0], [dy / d, dx, 0], [0, 0, 1]], dtype=t)
    return Gr, Gz


def initialise(mu, P, count, z, noise, t):
    """Slot ``count`` from observation z, in place (mu, P of dtype t, full size)."""
    lm, dx, dy = inverse_model(mu[:3], z, t)
    Gr, Gz = init_jacobians(mu[:3], z, t)
    r0 = 3 + 3 * count
    mu[r0:r0 + 3] = lm
    Pr = P[:3, :r0]
    rows = np.stack([Pr[0] - dy * Pr[2], Pr[1] + dx * Pr[2], Pr[2]])
    P[r0:r0 + 3, :r0] = rows
    P[:r0, r0:r0 + 3] = rows.T
    M = rows[:, :3]                                      # G_r P_rr
    D = np.stack([M[:, 0] - dy * M[:, 2], M[:, 1] + dx * M[:, 2], M[:, 2]], axis=1)
    D = D + Gz @ np.diag(scan_r(t(z[0]), noise, t)) @ Gz.T
    il = np.tril_indices(3)
    D.T[il] = D[il]                                      # the lower triangle, mirrored
    P[r0:r0 + 3, r0:r0 + 3] = D


# ------------------------------------------------------------------ update
def update_f64(mu, P, ids, obs, noise):
    """The update half of ekf_oracle.ekfslam_step (float64) on (mu, P)."""
    n, k = mu.size, len(ids)
    H = np.zeros((3 * k, n))
    innov = np.zeros(3 * k)
    Rb = np.zeros((3 * k, 3 * k))
    for t, (j, o) in enumerate(zip(ids, obs)):
        sl = slice(3 + 3 * j, 6 + 3 * j)
        Hr, Hl = eo.scan_jacobian(mu[:3], mu[sl])
        H[3 * t:3 * t + 3, :3] = Hr
        H[3 * t:3 * t + 3, sl] = Hl
        e = o - eo.scan_predict(mu[:3], mu[sl])
        e[1], e[2] = eo.wrap_angle(e[1]), eo.wrap_angle(e[2])
        innov[3 * t:3 * t + 3] = e
        Rb[3 * t:3 * t + 3, 3 * t:3 * t + 3] = eo.scan_cov(o[0], *noise)
    PHt = P @ H.T
    S = H @ PHt + Rb
    K = PHt @ np.linalg.inv(S)
    mu = mu + K @ innov
    mu[2] = eo.wrap_angle(mu[2])
    P = P - K @ S @ K.T
    return mu, 0.5 * (P + P.T)


def observe(mu, P, count, cap, obs, log_p_new, noise=NOISE, t=np.float64):
    """One slam_ekfslam_observe from the float64 state (mu, P, count), full
    size n = 3 + 3 cap with a zero tail.  Returns a dict: mu, P (dtype t, full
    size), count, assoc, scores, margin."""
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 3)
    mu = np.asarray(mu, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    l = scores(mu, P, count, obs, noise, t)
    assoc, margin = choose(l, log_p_new, count, cap)
    mu_n, P_n = mu.astype(t), P.astype(t)
    m = np.flatnonzero(assoc >= 0)
    if m.size:
        na = 3 + 3 * count
        if t is np.float64:
            mu_a, P_a = update_f64(mu[:na], P[:na, :na], assoc[m], obs[m], noise)
        else:
            mu_a, P_a = er.update(mu[:na], P[:na, :na], assoc[m], obs[m], noise)
        mu_n[:na], P_n[:na, :na] = mu_a, P_a
    for i in np.flatnonzero(assoc == NEW):
        initialise(mu_n, P_n, count, obs[i], noise, t)
        count += 1
    return dict(mu=mu_n, P=P_n, count=count, assoc=assoc, scores=l, margin=margin)


def predict(mu, P, count, control):
    """The float64 oracle's prediction on the active prefix."""
    na = 3 + 3 * count
    mu, P = mu.copy(), P.copy()
    mu[:na], P[:na, :na] = eo.ekfslam_predict(mu[:na], P[:na, :na], control, DT, Q_ROBOT)
    return mu, P


# ------------------------------------------------------------------ worlds
CONTROL = (10.0 * np.deg2rad(10.0), np.deg2rad(10.0))
X0 = np.array([10.0, 0.0, np.pi / 2])
P0_RR = np.diag([1e-4, 1e-4, 1e-6])

#        seed, landmarks, range, cap, p_new, steps
WORLDS = {"A": (3, 20, 9.0, 32, 0.1, 100),
          "B": (3, 20, 9.0, 6, 0.1, 100),
          "C": (7, 150, 12.0, 160, 0.1, 60)}


def make_scans(seed, n_lm, view, steps):
    """Landmarks (uniform +-15 m, heading +-pi), the robot on the reference's
    circle, and per step the noisy triples of the landmarks in range (at most
    40, by landmark index).  Returns (landmarks, [obs], [ids])."""
    rs = np.random.RandomState(seed)
    lm = np.column_stack([rs.uniform(-15, 15, (n_lm, 2)), rs.uniform(-np.pi, np.pi, n_lm)])
    pose = X0.copy()
    scans, ids = [], []
    for _ in range(steps):
        pose = eo.ekf_motion(pose, DT, *CONTROL)
        near = np.flatnonzero(np.hypot(lm[:, 0] - pose[0], lm[:, 1] - pose[1]) <= view)[:MAX_OBS]
        z = np.array([eo.scan_predict(pose, lm[j]) for j in near]).reshape(-1, 3)
        z[:, 0] *= 1 + rs.normal(0, 0.01, near.size)
        z[:, 1:] += rs.normal(0, 0.01, (near.size, 2))
        z[:, 1], z[:, 2] = wrap(z[:, 1], np.float64), wrap(z[:, 2], np.float64)
        scans.append(z)
        ids.append(near)
    return lm, scans, ids


def empty_state(cap):
    n = 3 + 3 * cap
    mu, P = np.zeros(n), np.zeros((n, n))
    mu[:3] = X0
    P[:3, :3] = P0_RR
    return mu, P


class Run:
    """A world run three ways, computed once: the float64 chain on its own
    state (``f64``: per step the input state, the predicted state and the
    result), the long-double step from each of the float64 chain's predicted
    states (``ld``: lockstep), and the long-double chain on its own state
    (``ld_free``: final state only, and ``free_spread`` -- the largest distance
    between the two chains over the run, (P relative to max |P|, mu absolute))."""

    def __init__(self, name, p_new=None, free=True):
        seed, n_lm, view, cap, pn, steps = WORLDS[name]
        self.cap, self.p_new = cap, pn if p_new is None else p_new
        self.log_p_new = float(np.log(self.p_new))
        self.lm, self.scans, self.ids = make_scans(seed, n_lm, view, steps)
        self.seen = len(set(np.concatenate(self.ids).tolist()))
        mu, P = empty_state(cap)
        count = 0
        self.f64, self.ld = [], []
        for z in self.scans:
            mu_p, P_p = predict(mu, P, count, CONTROL)
            r = observe(mu_p, P_p, count, cap, z, self.log_p_new)
            self.f64.append(dict(mu0=mu, P0=P, count0=count, mu_p=mu_p, P_p=P_p, obs=z, **r))
            self.ld.append(observe(mu_p, P_p, count, cap, z, self.log_p_new, t=LD))
            mu, P, count = r["mu"], r["P"], r["count"]
        if free:
            mu, P = empty_state(cap)
            count = 0
            sp_P = sp_mu = 0.0
            self.free_assoc = []
            for z, f in zip(self.scans, self.f64):
                mu_p, P_p = predict(mu, P, count, CONTROL)
                r = observe(mu_p, P_p, count, cap, z, self.log_p_new, t=LD)
                self.free_assoc.append(r["assoc"])
                if r["count"] == f["count"]:
                    sp_P = max(sp_P, float(np.abs(r["P"] - f["P"]).max() / np.abs(f["P"]).max()))
                    sp_mu = max(sp_mu, float(np.abs(r["mu"] - f["mu"]).max()))
                mu, P, count = r["mu"].astype(np.float64), r["P"].astype(np.float64), r["count"]
            self.ld_free = dict(mu=r["mu"], P=r["P"], count=count)
            self.free_spread = (sp_P, sp_mu)

    @property
    def decisions(self):
        return int(sum(len(z) for z in self.scans))

    @property
    def final_count(self):
        return self.f64[-1]["count"]

    def precondition(self):
        """(decisions identical in float64 and long double from every step's
        input state, smallest finite margin over both)."""
        same = all(np.array_equal(a["assoc"], b["assoc"]) and a["count"] == b["count"]
                   for a, b in zip(self.f64, self.ld))
        mg = np.concatenate([s["margin"] for s in self.f64 + self.ld])
        mg = mg[np.isfinite(mg)]
        return same, float(mg.min()) if mg.size else np.inf


@functools.lru_cache(maxsize=None)
def run(name, p_new=None, free=True):
    return Run(name, p_new, free)


def step_spread(f, l):
    """The float64 step's distance from the long-double step, same predicted
    state: (scores absolute, P relative to ``p_scale``, mu absolute)."""
    sc = float(np.abs(np.nan_to_num(f["scores"] - l["scores"])).max()) if f["scores"].size else 0.0
    return (sc, float(np.abs(f["P"] - l["P"]).max()) / p_scale(l),
            float(np.abs(f["mu"] - l["mu"]).max()))


def p_scale(l):
    """max |P| of a step's long-double result: the unit of the P bars (a step
    that initialises landmarks holds entries far above the predicted state's)."""
    return float(np.abs(l["P"]).max())


def bar(spread):
    """ekfslam_ref.bars' rule."""
    return max(1e-11, 64 * spread)
