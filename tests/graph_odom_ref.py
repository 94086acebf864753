"""TEST INFRASTRUCTURE -- NumPy restatement of the odometry edges of the graph
estimator, built on oracle/graph_oracle.py and
tests/graph_robust_ref.py.

An odometry edge ties pose b (earlier) to pose a with a measured relative
motion rel = (zx, zy, ztheta) in the axes of pose b and standard deviations
sigma.  With c = cos(theta_b), s = sin(theta_b), dx = x_a - x_b, dy = y_a - y_b:

  err   = (c dx + s dy - zx, -s dx + c dy - zy, wrap(wrap(theta_a - theta_b) - ztheta))
  Omega = diag(1 / sigma^2)
  J_b   = [[-c, -s, -s dx + c dy], [s, -c, -c dx - s dy], [0, 0, -1]]
  J_a   = [[ c,  s, 0], [-s, c, 0], [0, 0, 1]]

and the 42 values are those of a landmark edge.  Odometry edges are never
down-weighted: w = 1 and rho = chi2 under every robust kind.  The edge set is
the concatenation, landmark edges first.

Odometry rows: [t_bfr, pose_bfr, t_aft, pose_aft, zx, zy, ztheta, sx, sy, stheta].
"""
from __future__ import annotations

import functools

import numpy as np

import graph_oracle as go
import graph_robust_ref as rr
from pf_oracle import wrap_angle

SIGMA = (0.02, 0.02, 0.01)          # the odometry noise of the 72-pose experiment


def relpose(xb, xa):
    """Pose a in the axes of pose b: (c dx + s dy, -s dx + c dy, wrap(dtheta))."""
    xb = np.asarray(xb, dtype=np.float64).reshape(3)
    xa = np.asarray(xa, dtype=np.float64).reshape(3)
    c, s = np.cos(xb[2]), np.sin(xb[2])
    dx, dy = xa[0] - xb[0], xa[1] - xb[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, wrap_angle(xa[2] - xb[2])])


def odom_err_info(row, poses):
    """err (3,), Omega (3, 3), J_b, J_a of one odometry row at ``poses``."""
    pb, pa = int(row[1]), int(row[3])
    z, sig = np.asarray(row[4:7], dtype=np.float64), np.asarray(row[7:10], dtype=np.float64)
    xb, xa = poses[pb], poses[pa]
    c, s = np.cos(xb[2]), np.sin(xb[2])
    dx, dy = xa[0] - xb[0], xa[1] - xb[1]
    err = np.array([c * dx + s * dy - z[0], -s * dx + c * dy - z[1],
                    wrap_angle(wrap_angle(xa[2] - xb[2]) - z[2])])
    info = np.diag(1.0 / (sig * sig))
    jb = np.array([[-c, -s, -s * dx + c * dy], [s, -c, -c * dx - s * dy], [0.0, 0.0, -1.0]])
    ja = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    return err, info, jb, ja


def linearize_odom(odom, poses):
    """(n, 42): BB, BA, AB, AA (row-major 3x3), b_B, b_A of every odometry row."""
    out = np.empty((len(odom), 42))
    for i, row in enumerate(odom):
        err, info, jb, ja = odom_err_info(row, poses)
        parts = [jb.T @ info @ jb, jb.T @ info @ ja, ja.T @ info @ jb, ja.T @ info @ ja,
                 jb.T @ info @ err, ja.T @ info @ err]
        out[i] = np.concatenate([m.ravel() for m in parts])
    return out


def chi2_weights(edges, odom, poses, kind=None, param=None):
    """(chi2, w, rho) over the mixed set, landmark edges first; the odometry
    edges have w = 1 and rho = chi2 whatever the kind."""
    c_lm, w_lm, r_lm = rr.chi2_weights(edges, poses, kind, param) if len(edges) else (np.empty(0),) * 3
    c_od = np.empty(len(odom))
    for i, row in enumerate(odom):
        err, info, _, _ = odom_err_info(row, poses)
        c_od[i] = err @ (info @ err)
    return (np.concatenate([c_lm, c_od]), np.concatenate([w_lm, np.ones(len(odom))]),
            np.concatenate([r_lm, c_od]))


def _endpoints(edges, odom):
    """Rows carrying the two times where graph_oracle.assemble reads them."""
    ends = np.zeros((len(edges) + len(odom), go.EDGE_FIELDS))
    if len(edges):
        ends[:len(edges), 0], ends[:len(edges), 5] = edges[:, 0], edges[:, 5]
    if len(odom):
        ends[len(edges):, 0], ends[len(edges):, 5] = odom[:, 0], odom[:, 2]
    return ends


def linearize(edges, odom, poses, kind=None, param=None):
    """(blocks (E, 42) weighted, chi2, w) of the mixed set."""
    chi2, w, _ = chi2_weights(edges, odom, poses, kind, param)
    blk_lm = go.linearize(edges, poses) if len(edges) else np.empty((0, 42))
    blocks = np.concatenate([blk_lm, linearize_odom(odom, poses)]) * w[:, None]
    return blocks, chi2, w


def update_est_pose(edges, odom, poses, kind=None, param=None):
    """graph_robust_ref.update_est_pose over the mixed set.  Returns (stats,
    new poses, H, b, times, chi2, w, delta)."""
    poses = np.array(poses, dtype=np.float64, copy=True)
    edges = np.asarray(edges, dtype=np.float64).reshape(len(edges), go.EDGE_FIELDS)
    odom = np.asarray(odom, dtype=np.float64).reshape(len(odom), 10)
    blocks, chi2, w = linearize(edges, odom, poses, kind, param)
    times, H, b = go.assemble(_endpoints(edges, odom), blocks)
    n = 3 * len(times)
    if n <= 3:
        return np.zeros(4), poses, H, b[:, 0], times, chi2, w, np.zeros(n)
    det = np.linalg.det(H)
    cond = np.linalg.cond(H)
    if 0.1 < det and cond < 10 ** 15:                       # the reference's gate
        delta = -np.linalg.inv(H) @ b
        for i, t in enumerate(times):
            poses[t, 0] += delta[i * 3, 0]
            poses[t, 1] += delta[i * 3 + 1, 0]
            poses[t, 2] = wrap_angle(poses[t, 2] + delta[i * 3 + 2, 0])
        return (np.array([1.0, float((delta.T @ delta)[0, 0]), det, cond]), poses, H, b[:, 0],
                times, chi2, w, delta[:, 0])
    return np.array([0.0, 0.0, det, cond]), poses, H, b[:, 0], times, chi2, w, np.zeros(n)


def gauss_newton(edges, odom, poses, kind=None, param=None, delta_sum_th=0.01, max_iter=50):
    """The estimator's loop over the mixed set.  Returns (poses, stats (n_iter, 4))."""
    st = []
    dsum = delta_sum_th
    while delta_sum_th <= dsum and len(st) < max_iter:
        s, poses = update_est_pose(edges, odom, poses, kind, param)[:2]
        st.append(s)
        dsum = s[1]
    return poses, np.array(st).reshape(-1, 4)


def odom_rows(rec):
    """slam_graph_odom records -> odometry rows."""
    return np.column_stack([rec["time_bfr"], rec["pose_bfr"], rec["time_aft"], rec["pose_aft"],
                            rec["rel"], rec["sigma"]]).astype(np.float64).reshape(len(rec), 10)


@functools.lru_cache(maxsize=None)
def odometry(seed):
    """The recipe of DESIGN 8.4 on the seed's graph: one odometry edge per consecutive
    pose pair, rel = relpose(truth[k-1], truth[k]) + SIGMA * standard normals of
    RandomState(1000 + seed), drawn in order k = 1 .. T-1 (read-only records)."""
    from slamhip.graph import circle_graph_odometry
    truth = rr.corrupted_graph(seed)[1]
    rec = circle_graph_odometry(truth, SIGMA, seed)
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def cpu_run(seed, kind, param, corrupted, with_odom):
    """Gauss-Newton of the restatement on the seed's graph with or without its
    odometry edges (once per session; read-only).  Returns (poses, stats)."""
    init, _, rec, cor, _ = rr.corrupted_graph(seed)
    edges = rr.edge_rows(cor if corrupted else rec)
    odom = odom_rows(odometry(seed)) if with_odom else np.empty((0, 10))
    poses, st = gauss_newton(edges, odom, init, kind, param)
    for a in (poses, st):
        a.setflags(write=False)
    return poses, st
