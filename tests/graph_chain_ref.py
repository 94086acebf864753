"""TEST INFRASTRUCTURE -- NumPy restatement of the chain preconditioner of the
graph estimator's PCG and of the PCG itself.

The rows are the system's times in order, nt of them; S is the segment length in
poses.  D_r is the diagonal block of row r, U_r the block (r, r+1) if that slot
exists and floor(r / S) == floor((r + 1) / S), else 0.  M's lower blocks are
U_r^T (H's own (r+1, r) block is not read).

  factor   S_r = D_r at a segment start, else D_r - U_{r-1}^T G_{r-1}
           Sinv_r = inv(S_r),  G_r = Sinv_r U_r
  apply    forward   y_r = r_r - G_{r-1}^T y_{r-1}   (y_r = r_r at a segment start)
           backward  z_r = Sinv_r y_r - G_r z_{r+1}  (z_r = Sinv_r y_r at a segment end)

S = 1 is block-Jacobi.  A pivot S_r is bad when a leading minor is not positive
or a value is not finite.  The PCG is the device's recurrences (p = z + beta p,
q = H z + beta q, the test r.r <= tol^2 r0.r0 before iteration k's direction)
with NumPy's summation order.
"""
from __future__ import annotations

import functools

import numpy as np

SEGMENTS = (1, 2, 4, 8, 16, 32, 64)


def bsr_from_dense(H):
    """(rows, cols, vals (n_slots, 3, 3)) of the non-zero 3x3 blocks of a dense H
    and its diagonal, sorted by r * nt + c like the handle's slots."""
    nt = H.shape[0] // 3
    blk = H.reshape(nt, 3, nt, 3).transpose(0, 2, 1, 3)
    keep = np.any(blk != 0.0, axis=(2, 3)) | np.eye(nt, dtype=bool)
    rows, cols = np.nonzero(keep)
    return rows.astype(np.int64), cols.astype(np.int64), blk[rows, cols].copy()


def dense_from_bsr(rows, cols, vals, nt):
    H = np.zeros((3 * nt, 3 * nt))
    for r, c, v in zip(rows, cols, vals):
        H[3 * r:3 * r + 3, 3 * c:3 * c + 3] = v
    return H


def chain_blocks(rows, cols, vals, nt, S):
    """D (nt, 3, 3), U (nt, 3, 3) (zero where M has no (r, r+1) block) and the
    number of off-diagonal blocks used."""
    D = np.zeros((nt, 3, 3))
    U = np.zeros((nt, 3, 3))
    used = 0
    for r, c, v in zip(rows, cols, vals):
        if r == c:
            D[r] = v
        elif c == r + 1 and r // S == c // S:
            U[r] = v
            used += 1
    return D, U, used


def build_m(rows, cols, vals, nt, S):
    """M as a dense matrix."""
    D, U, _ = chain_blocks(rows, cols, vals, nt, S)
    M = np.zeros((3 * nt, 3 * nt))
    for r in range(nt):
        M[3 * r:3 * r + 3, 3 * r:3 * r + 3] = D[r]
        if r + 1 < nt:
            M[3 * r:3 * r + 3, 3 * r + 3:3 * r + 6] = U[r]
            M[3 * r + 3:3 * r + 6, 3 * r:3 * r + 3] = U[r].T
    return M


def _bad_pivot(P):
    minors = (P[0, 0], np.linalg.det(P[:2, :2]), np.linalg.det(P))
    return not (np.all(np.isfinite(P)) and all(m > 0.0 for m in minors))


def factor(rows, cols, vals, nt, S):
    """(Sinv (nt, 3, 3), G (nt, 3, 3), off-diagonal blocks used, bad pivots)."""
    D, U, used = chain_blocks(rows, cols, vals, nt, S)
    Sinv = np.zeros((nt, 3, 3))
    G = np.zeros((nt, 3, 3))
    bad = 0
    for r in range(nt):
        P = D[r] if r % S == 0 else D[r] - U[r - 1].T @ G[r - 1]
        bad += _bad_pivot(P)
        with np.errstate(all="ignore"):
            try:
                Sinv[r] = np.linalg.inv(P)
            except np.linalg.LinAlgError:
                Sinv[r] = np.nan
            G[r] = Sinv[r] @ U[r]
    return Sinv, G, used, bad


def apply(Sinv, G, S, r):
    """z = M^-1 r."""
    nt = len(Sinv)
    y = np.array(r, dtype=np.float64).reshape(nt, 3)
    for k in range(nt):
        if k % S:
            y[k] = y[k] - G[k - 1].T @ y[k - 1]
    z = np.empty_like(y)
    for k in range(nt - 1, -1, -1):
        z[k] = Sinv[k] @ y[k]
        if (k + 1) % S and k + 1 < nt:
            z[k] = z[k] - G[k] @ z[k + 1]
    return z.reshape(-1)


def pcg(H, b, precond, tol=1e-10, max_iter=20000):
    """H x = -b by the device's recurrences with ``precond`` (a function r -> z).
    Returns (x, iterations, status): status 1 converged, 2 not positive definite
    along p, 3 max_iter."""
    x = np.zeros(len(b))
    r = -np.asarray(b, dtype=np.float64)
    z = precond(r)
    p = np.zeros_like(x)
    q = np.zeros_like(x)
    rr0 = rho_prev = 0.0
    for k in range(max_iter + 1):
        rho, rr = float(r @ z), float(r @ r)
        if k == 0:
            rr0 = rr
            if rr == 0.0:
                return x, k, 1
        else:
            if rr <= tol * tol * rr0:
                return x, k, 1
            if k >= max_iter:
                return x, k, 3
        beta = rho / rho_prev if k else 0.0
        p = z + beta * p
        q = H @ z + beta * q
        pq = float(p @ q)
        if not pq > 0.0:
            return x, k, 2
        alpha = rho / pq
        x = x + alpha * p
        r = r - alpha * q
        z = precond(r)
        rho_prev = rho
    return x, max_iter, 3


def chain_precond(H_bsr, nt, S):
    """r -> M^-1 r of the chain preconditioner with segment S on (rows, cols, vals)."""
    Sinv, G, _, _ = factor(*H_bsr, nt, S)
    return lambda r: apply(Sinv, G, S, r)


# ------------------------------------------------------------------ the cases
# name -> (poses (T, 3), pair records, odometry records, robust kind or None):
# the systems the apply is checked on, here against np.linalg.solve and in
# test_gpu_graph_chain.py on the device.
ODOM_ONLY = (2, 3, 63, 64, 65, 128, 129, 200)
GAPS = ((10, 11), (63, 64))
CASES = tuple("odom%d" % n for n in ODOM_ONLY) + ("mixed72", "mixed200", "gaps", "even_times", "cauchy")


@functools.lru_cache(maxsize=None)
def _circle(n_poses, seed):
    from slamhip.graph import circle_graph, circle_graph_odometry
    import graph_odom_ref as gr
    init, truth, rec = circle_graph(n_poses, n_landmarks=16, seed=seed)
    od = circle_graph_odometry(truth, gr.SIGMA, seed)
    for a in (init, truth, rec, od):
        a.setflags(write=False)
    return init, truth, rec, od


def case(name):
    from slamhip.graph import EDGE_DTYPE
    none = np.zeros(0, dtype=EDGE_DTYPE)
    if name.startswith("odom"):
        nt = int(name[4:])
        init, _, _, od = _circle(200, 3)
        return init[:nt], none, od[:nt - 1], None
    if name in ("mixed72", "cauchy"):
        init, _, rec, od = _circle(72, 5)
        return init, rec, od, ("cauchy", 2.0) if name == "cauchy" else None
    init, _, rec, od = _circle(200, 3)
    if name == "mixed200":
        return init, rec, od, None
    if name == "gaps":
        # no edge of either kind between rows 10, 11 and between rows 63, 64: a missing
        # slot inside a segment and at a segment boundary (the loop edges keep H connected)
        keep = np.ones(len(rec), dtype=bool)
        for a, b in GAPS:
            keep &= ~((rec["time_bfr"] == a) & (rec["time_aft"] == b))
        return init, rec[keep], od[~np.isin(od["time_bfr"], [a for a, _ in GAPS])], None
    if name == "even_times":
        # 70 rows at the times 0, 2, 4, ..: adjacent rows, times that are not
        od2 = od[:69].copy()
        for f in ("time_bfr", "pose_bfr", "time_aft", "pose_aft"):
            od2[f] *= 2
        poses = np.zeros((140, 3))
        poses[::2] = init[:70]
        return poses, none, od2, None
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case_system(name):
    """(H, b) of the case by the restatements (read-only)."""
    import graph_odom_ref as gr
    import graph_robust_ref as rr
    poses, rec, od, robust = case(name)
    kind, param = robust if robust else (None, None)
    edges = rr.edge_rows(rec).reshape(len(rec), 11)
    H, b = _assemble(edges, gr.odom_rows(od), poses, kind, param)
    for a in (H, b):
        a.setflags(write=False)
    return H, b


@functools.lru_cache(maxsize=None)
def table_system(T, with_odom):
    """The system of DESIGN 8.5's CPU table (read-only): circle_graph(T,
    n_landmarks=64, seed=0, odom_noise=0.002), with its odometry edges
    circle_graph_odometry(truth, (0.02, 0.02, 0.01), 0) or without, linearised
    at the initial poses and assembled with the 1e4 anchor.  Returns (H, b)."""
    import graph_odom_ref as gr
    import graph_robust_ref as rr
    from slamhip.graph import circle_graph, circle_graph_odometry
    init, truth, rec = circle_graph(T, n_landmarks=64, seed=0, odom_noise=0.002)
    edges = rr.edge_rows(rec)
    odom = gr.odom_rows(circle_graph_odometry(truth, gr.SIGMA, 0)) if with_odom else np.empty((0, 10))
    H, b = _assemble(edges, odom, init)
    for a in (H, b):
        a.setflags(write=False)
    return H, b


def _assemble(edges, odom, init, kind=None, param=None):
    import graph_odom_ref as gr
    import graph_oracle as go
    blocks = gr.linearize(edges, odom, init, kind, param)[0]
    _, H, b = go.assemble(gr._endpoints(edges, odom), blocks)
    return H, b[:, 0].copy()


@functools.lru_cache(maxsize=None)
def table_iterations(T, with_odom, S):
    """PCG iterations (tol 1e-10) on table_system with block-Jacobi (S = 0) or
    the chain preconditioner with segment S (S >= nt: the whole chain)."""
    H, b = table_system(T, with_odom)
    nt = len(b) // 3
    pre = chain_precond(bsr_from_dense(H), nt, 1 if S == 0 else S)
    _, it, status = pcg(H, b, pre, 1e-10)
    assert status == 1, (T, with_odom, S, status)
    return it
