"""TEST INFRASTRUCTURE -- NumPy restatement of the robust edge weights of the
graph estimator, built on oracle/graph_oracle.py's functions.

For edge e, err and Omega are what graph_oracle.linearize_edge (the device's
linearise kernel) forms; chi2_e = err^T Omega err, and

  kind       weight w                                   robust cost rho
  none       1                                          chi2
  huber(k)   1 for chi2 <= k^2, else k / sqrt(chi2)     chi2, else 2 k sqrt(chi2) - k^2
  cauchy(k)  1 / (1 + chi2 / k^2)                       k^2 ln(1 + chi2 / k^2)
  dcs(P)     s^2, s = min(1, 2 P / (P + chi2))          s^2 chi2 + P (1 - s)^2

All six blocks and both right-hand-side parts of the edge are multiplied by w
(iteratively re-weighted least squares: the weights are recomputed at every
linearisation).
"""
from __future__ import annotations

import functools

import numpy as np

import graph_oracle as go
from pf_oracle import wrap_angle

KINDS = ("none", "huber", "cauchy", "dcs")
# the issue's cases: (kind, parameter)
CASES = (("huber", 1.0), ("huber", 2.0), ("cauchy", 2.0), ("dcs", 5.0))


def weight_cost(chi2, kind, param):
    """(w, rho) of chi2 (array) under ``kind``."""
    chi2 = np.asarray(chi2, dtype=np.float64)
    if kind in (None, "none"):
        return np.ones_like(chi2), chi2.copy()
    k = float(param)
    if kind == "huber":
        out = chi2 > k * k
        root = np.sqrt(np.where(out, chi2, 1.0))
        return np.where(out, k / root, 1.0), np.where(out, 2.0 * k * root - k * k, chi2)
    if kind == "cauchy":
        t = 1.0 + chi2 / (k * k)
        return 1.0 / t, k * k * np.log(t)
    if kind == "dcs":
        s = np.minimum(1.0, 2.0 * k / (k + chi2))
        return s * s, s * s * chi2 + k * (1.0 - s) ** 2
    raise ValueError(kind)


def edge_err_info(edge, poses):
    """err (3,) and Omega (3, 3) of one edge, as graph_oracle.linearize_edge forms them."""
    tb, pb, db, ab, ob, ta, pa, da, aa, oa = edge[:10]
    xb = np.array(poses[int(pb)], dtype=np.float64).reshape(3, 1)
    xa = np.array(poses[int(pa)], dtype=np.float64).reshape(3, 1)
    rel = xa - xb
    rel[2, 0] = wrap_angle(rel[2, 0])
    la = go.landmark_frame(da, aa, oa)
    lb = go.landmark_frame(db, ab, ob)
    px = la[0] * np.cos(la[1]) - lb[0] * np.cos(lb[1])
    py = la[0] * np.sin(la[1]) - lb[0] * np.sin(lb[1])
    pt = wrap_angle(la[2] - lb[2])
    err = rel - np.array([[px], [py], [pt]])
    err[2, 0] = wrap_angle(err[2, 0])
    ca = go.cov_to_world(go.measurement_cov(da), aa, xa[2, 0])
    cb = go.cov_to_world(go.measurement_cov(db), ab, xb[2, 0])
    return err[:, 0], np.linalg.inv(ca + cb)


def chi2_weights(edges, poses, kind, param):
    """(chi2, w, rho), one entry per edge row, at ``poses`` (T, 3)."""
    chi2 = np.empty(len(edges))
    for i, e in enumerate(edges):
        err, info = edge_err_info(e, poses)
        chi2[i] = err @ (info @ err)
    w, rho = weight_cost(chi2, kind, param)
    return chi2, w, rho


def update_est_pose(edges, poses, kind=None, param=None):
    """graph_oracle.update_est_pose with every edge's 42 values scaled by its
    weight.  Returns (stats, new poses, H, b, times, chi2, w)."""
    poses = np.array(poses, dtype=np.float64, copy=True)
    chi2, w, _ = chi2_weights(edges, poses, kind, param)
    blocks = go.linearize(edges, poses) * w[:, None]
    times, H, b = go.assemble(edges, blocks)
    if len(times) * 3 <= 3:
        return np.zeros(4), poses, H, b[:, 0], times, chi2, w
    det = np.linalg.det(H)
    cond = np.linalg.cond(H)
    if 0.1 < det and cond < 10 ** 15:                       # the reference's gate
        delta = -np.linalg.inv(H) @ b
        for i, t in enumerate(times):
            poses[t, 0] += delta[i * 3, 0]
            poses[t, 1] += delta[i * 3 + 1, 0]
            poses[t, 2] = wrap_angle(poses[t, 2] + delta[i * 3 + 2, 0])
        return (np.array([1.0, float((delta.T @ delta)[0, 0]), det, cond]), poses, H, b[:, 0],
                times, chi2, w)
    return np.array([0.0, 0.0, det, cond]), poses, H, b[:, 0], times, chi2, w


def gauss_newton(edges, poses, kind=None, param=None, delta_sum_th=0.01, max_iter=50):
    """The estimator's loop: update while delta_sum_th <= sum(delta^2), at most
    max_iter times.  Returns (poses, stats (n_iter, 4))."""
    st = []
    dsum = delta_sum_th
    while delta_sum_th <= dsum and len(st) < max_iter:
        s, poses = update_est_pose(edges, poses, kind, param)[:2]
        st.append(s)
        dsum = s[1]
    return poses, np.array(st).reshape(-1, 4)


def edge_rows(rec):
    """slam_graph_edge records -> oracle edge rows (landmark column 0)."""
    return np.column_stack([rec["time_bfr"], rec["pose_bfr"], rec["obs_bfr"], rec["time_aft"],
                            rec["pose_aft"], rec["obs_aft"], np.zeros(len(rec))]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def corrupted_graph(seed, n_poses=72, n_landmarks=16, frac=0.1):
    """The issue's recipe: circle_graph(72, n_landmarks=16, seed), and in one
    edge in ten obs_aft replaced by the obs_aft of another edge (a wrong
    pairing).  Returns (init, truth, clean records, corrupted records, bad mask)."""
    from slamhip.graph import circle_graph
    init, truth, rec = circle_graph(n_poses, n_landmarks=n_landmarks, seed=seed)
    E = len(rec)
    rs = np.random.RandomState(100 + seed)
    bad = rs.choice(E, int(frac * E), replace=False)
    src = rs.permutation(E)[:len(bad)]
    cor = rec.copy()
    cor["obs_aft"][bad] = rec["obs_aft"][src]
    mask = np.zeros(E, dtype=bool)
    mask[bad] = True
    for a in (init, truth, rec, cor, mask):
        a.setflags(write=False)
    return init, truth, rec, cor, mask


def position_rms(p, q):
    return float(np.sqrt(np.mean(np.sum((p[:, :2] - q[:, :2]) ** 2, axis=1))))


@functools.lru_cache(maxsize=None)
def cpu_run(seed, kind, param, corrupted=True):
    """Gauss-Newton of the restatement on the seed's graph (computed once per
    session, shared by the tests; the arrays are read-only).  Returns (poses,
    stats, chi2, w) with chi2 and w evaluated at the final poses."""
    init, _, rec, cor, _ = corrupted_graph(seed)
    edges = edge_rows(cor if corrupted else rec)
    poses, st = gauss_newton(edges, init, kind, param)
    chi2, w, _ = chi2_weights(edges, poses, kind, param)
    for a in (poses, st, chi2, w):
        a.setflags(write=False)
    return poses, st, chi2, w
