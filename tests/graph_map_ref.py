"""TEST INFRASTRUCTURE -- NumPy restatement of the landmark map of the graph
estimator, built on oracle/graph_oracle.py, and the test world of
its experiments.

Conditional on the poses the landmarks are independent; landmark l is the
information-weighted fusion of its half-edges.  For half-edge k = (time, pose,
landmark, (d, dir, orient)) with the observing pose's estimate (x, y, theta):

  ang  = dir + theta - pi/2                     (graph_oracle.cov_to_world's angle)
  L_k  = (x + d cos ang, y + d sin ang)
  C_k  = the upper 2x2 of cov_to_world(measurement_cov(d), dir, theta)     W_k = C_k^-1
  Lam  = sum_k W_k        eta = sum_k W_k (L_k - L_k0)      k0: the first half-edge as recorded
  cov  = Lam^-1           mean = L_k0 + cov eta
  chi2_k = (L_k - mean)^T W_k (L_k - mean)      chi2_l = sum_k chi2_k

The orientation does not enter.  The sums are folded sequentially in recording
order.  A landmark nobody saw has count 0 and NaN mean, cov and chi2; a
half-edge whose landmark id is outside [0, n_landmarks) is ignored and its
chi2_k is NaN.

Half-edge rows: [time, pose_id, landmark, dist, dir, orient].
"""
from __future__ import annotations

import functools

import numpy as np

import graph_odom_ref as orf
import graph_oracle as go
from pf_oracle import HALF_PI, wrap_angle


def half_terms(row, poses):
    """(L_k (2,), C_k (2, 2), W_k (2, 2)) of one half-edge row at ``poses``."""
    x, y, th = poses[int(row[1])]
    d, a = row[3], row[4]
    ang = a + th - HALF_PI
    L = np.array([x + d * np.cos(ang), y + d * np.sin(ang)])
    C = go.cov_to_world(go.measurement_cov(d), a, th)[0:2, 0:2]
    return L, C, np.linalg.inv(C)


def landmark_map(halves, n_landmarks, poses):
    """(mean (NL, 2), cov (NL, 2, 2), count (NL,), chi2 (NL,), half_chi2 (n,))."""
    halves = np.asarray(halves, dtype=np.float64).reshape(-1, 6)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    mean = np.full((n_landmarks, 2), np.nan)
    cov = np.full((n_landmarks, 2, 2), np.nan)
    chi2 = np.full(n_landmarks, np.nan)
    count = np.zeros(n_landmarks, dtype=np.int64)
    half_chi2 = np.full(len(halves), np.nan)
    ids = halves[:, 2].astype(np.int64)
    for l in range(n_landmarks):
        ks = np.flatnonzero(ids == l)
        count[l] = len(ks)
        if not len(ks):
            continue
        terms = [half_terms(halves[k], poses) for k in ks]
        L0 = terms[0][0]
        lam, eta = np.zeros((2, 2)), np.zeros(2)
        for L, _, W in terms:                      # sequential, recording order
            lam = lam + W
            eta = eta + W @ (L - L0)
        cov[l] = np.linalg.inv(lam)
        mean[l] = L0 + cov[l] @ eta
        tot = 0.0
        for k, (L, _, W) in zip(ks, terms):
            r = L - mean[l]
            half_chi2[k] = r @ (W @ r)
            tot = tot + half_chi2[k]
        chi2[l] = tot
    return mean, cov, count, chi2, half_chi2


def map_rms(mean, landmarks):
    """RMS distance of the estimated landmarks (those seen) from the true ones."""
    seen = ~np.isnan(mean[:, 0])
    d = mean[seen] - np.asarray(landmarks)[seen]
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


def chi2_per_dof(count, chi2):
    """sum chi2_l over 2 (n_l - 1) degrees of freedom per landmark seen."""
    seen = count > 0
    return float(np.sum(chi2[seen]) / np.sum(2 * (count[seen] - 1)))


def compose(pose, rel):
    """The pose reached from ``pose`` by the relative motion ``rel`` in its axes."""
    c, s = np.cos(pose[2]), np.sin(pose[2])
    return np.array([pose[0] + c * rel[0] - s * rel[1], pose[1] + s * rel[0] + c * rel[1],
                     wrap_angle(pose[2] + rel[2])])


@functools.lru_cache(maxsize=None)
def world(seed, n_poses=72, n_landmarks=16):
    """The test world (read-only arrays): circle_graph's circle, ``n_landmarks``
    points on the 14 m ring, per pose t the noisy scan of graph_oracle.scan_sensor
    after np.random.seed(1000 * seed + t) as half-edges (t, t, id, obs), their
    pair edges, the odometry of DESIGN 8.4's recipe, and the start: the
    composition of the noisy steps from the first true pose.  The global NumPy
    stream is restored."""
    from slamhip.graph import circle_graph, circle_graph_odometry
    truth = circle_graph(n_poses, n_landmarks=n_landmarks, seed=seed)[1]
    la = np.linspace(0, 2 * np.pi, n_landmarks, endpoint=False)
    lm = np.column_stack([14 * np.cos(la), 14 * np.sin(la)])
    state = np.random.get_state()
    rows = []
    for t in range(n_poses):
        np.random.seed(1000 * seed + t)
        ids, _, noisy = go.scan_sensor(truth[t], lm, 15.0, np.deg2rad(80.0), go.R_DIST, go.R_DIR,
                                       go.R_ORIENT)
        rows += [[t, t, i, *o] for i, o in zip(ids, noisy)]
    np.random.set_state(state)
    halves = np.array(rows, dtype=np.float64).reshape(-1, 6)
    edges = go.edges_from_pairs(go.pairs_from_halves(halves, n_landmarks))
    odom = circle_graph_odometry(truth, orf.SIGMA, seed)
    start = np.empty_like(truth)
    start[0] = truth[0]
    for k in range(1, n_poses):
        start[k] = compose(start[k - 1], odom["rel"][k - 1])
    out = dict(truth=truth, landmarks=lm, halves=halves, edges=edges, odom=odom,
               odom_rows=orf.odom_rows(odom), start=start)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cpu_optimised(seed, n_poses=72, n_landmarks=16):
    """The restatement's Gauss-Newton with odometry on the test world, from its
    start (once per session; read-only).  Returns the optimised poses."""
    w = world(seed, n_poses, n_landmarks)
    poses, _ = orf.gauss_newton(w["edges"], w["odom_rows"], w["start"])
    poses.setflags(write=False)
    return poses
