"""Device graph-based SLAM: a handle on libslam_hip's slam_graph_* entry
points (TrajectoryEstimator's linearise-and-solve, graph_based_slam.py
:362-514, and the Gauss-Newton loop :685-715)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import GRAPH_COND, GRAPH_PRECOND, GRAPH_ROBUST, GRAPH_SOLVER, GraphConfig, check, dptr

# slam_graph_edge, 80 bytes
EDGE_DTYPE = np.dtype([("time_bfr", "<i8"), ("pose_bfr", "<i8"), ("time_aft", "<i8"),
                       ("pose_aft", "<i8"), ("obs_bfr", "<f8", (3,)), ("obs_aft", "<f8", (3,))])

# slam_graph_odom, 80 bytes: the index prefix of slam_graph_edge, then rel and sigma
ODOM_DTYPE = np.dtype([("time_bfr", "<i8"), ("pose_bfr", "<i8"), ("time_aft", "<i8"),
                       ("pose_aft", "<i8"), ("rel", "<f8", (3,)), ("sigma", "<f8", (3,))])


HALF_DTYPE = np.dtype([("time", "<i8"), ("pose", "<i8"), ("landmark", "<i8"), ("obs", "<f8", (3,))])


def half_array(halves):
    """Half-edge rows [time, pose_id, landmark, dist, dir, orient] (or HALF_DTYPE
    records) -> contiguous slam_graph_half records."""
    if not (isinstance(halves, np.ndarray) and halves.dtype == HALF_DTYPE):
        rows = np.asarray(halves, dtype=np.float64).reshape(-1, 6)
        rec = np.zeros(len(rows), dtype=HALF_DTYPE)
        rec["time"], rec["pose"], rec["landmark"] = rows[:, 0], rows[:, 1], rows[:, 2]
        rec["obs"] = rows[:, 3:6]
        halves = rec
    return np.ascontiguousarray(halves)


def pair_halves(halves, n_landmarks, device=0):
    """Robot.estimateOpticalTrajectory's pairing (graph_based_slam.py:697-703)
    on the device: ``halves`` rows [time, pose_id, landmark, dist, dir, orient]
    (or HALF_DTYPE records) in recording order -> slam_graph_edge records, in
    the reference's order (landmark, then itertools.combinations), each pair
    ordered as setPairObs orders it (:371-384)."""
    halves = half_array(halves)
    lib = _lib.load()
    n = C.c_int64(0)
    check(lib.slam_graph_pair_halves(len(halves), halves.ctypes.data_as(C.c_void_p),
                                     int(n_landmarks), int(device), C.byref(n), None),
          "slam_graph_pair_halves")
    out = np.zeros(n.value, dtype=EDGE_DTYPE)
    if n.value:
        check(lib.slam_graph_pair_halves(len(halves), halves.ctypes.data_as(C.c_void_p),
                                         int(n_landmarks), int(device), C.byref(n),
                                         out.ctypes.data_as(C.c_void_p)),
              "slam_graph_pair_halves")
    return out


def edge_array(rows):
    """Edge rows [t_bfr, pose_bfr, d, dir, orient, t_aft, pose_aft, d, dir, orient, (lm)]
    -> slam_graph_edge records (no rows: an empty record array)."""
    if len(rows) == 0:
        return np.zeros(0, dtype=EDGE_DTYPE)
    rows = np.asarray(rows, dtype=np.float64).reshape(len(rows), -1)
    out = np.zeros(len(rows), dtype=EDGE_DTYPE)
    out["time_bfr"] = rows[:, 0].astype(np.int64)
    out["pose_bfr"] = rows[:, 1].astype(np.int64)
    out["obs_bfr"] = rows[:, 2:5]
    out["time_aft"] = rows[:, 5].astype(np.int64)
    out["pose_aft"] = rows[:, 6].astype(np.int64)
    out["obs_aft"] = rows[:, 7:10]
    return out


def odom_array(rows):
    """Odometry rows [t_bfr, pose_bfr, t_aft, pose_aft, zx, zy, ztheta, sx, sy, stheta]
    -> slam_graph_odom records."""
    rows = np.asarray(rows, dtype=np.float64).reshape(len(rows), 10)
    out = np.zeros(len(rows), dtype=ODOM_DTYPE)
    for k, name in enumerate(("time_bfr", "pose_bfr", "time_aft", "pose_aft")):
        out[name] = rows[:, k].astype(np.int64)
    out["rel"] = rows[:, 4:7]
    out["sigma"] = rows[:, 7:10]
    return out


def relpose(xb, xa):
    """Pose ``xa`` in the axes of pose ``xb``: (c dx + s dy, -s dx + c dy,
    wrap(theta_a - theta_b)) with c, s = cos, sin of theta_b -- the ``rel`` of an
    odometry edge.  Unchanged under a rigid motion of both poses."""
    xb = np.asarray(xb, dtype=np.float64).reshape(3)
    xa = np.asarray(xa, dtype=np.float64).reshape(3)
    c, s = np.cos(xb[2]), np.sin(xb[2])
    dx, dy = xa[0] - xb[0], xa[1] - xb[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy,
                     np.mod(xa[2] - xb[2] + np.pi, 2 * np.pi) - np.pi])


class DeviceGraph:
    """Pose graph on one GPU.  Noise defaults = Robot's setNoiseParam(5, 2, 2)
    (graph_based_slam.py:604); anchor and gate = updateEstPose :475, :496."""

    def __init__(self, *, r_dist=0.05, r_dir=np.deg2rad(2.0), r_orient=np.deg2rad(2.0),
                 anchor=1e4, det_min=0.1, cond_max=1e15, solver="auto", pcg_tol=1e-10,
                 pcg_max_iter=20000, cond="margin", cond_tol=1e-5, cond_max_iter=3000, device=0,
                 robust=None):
        cfg = GraphConfig()
        cfg.r_dist, cfg.r_dir, cfg.r_orient = float(r_dist), float(r_dir), float(r_orient)
        cfg.anchor, cfg.det_min, cfg.cond_max = float(anchor), float(det_min), float(cond_max)
        cfg.pcg_tol, cfg.pcg_max_iter = float(pcg_tol), int(pcg_max_iter)
        cfg.solver = GRAPH_SOLVER[solver]
        cfg.cond_mode = GRAPH_COND[cond]
        cfg.cond_tol, cfg.cond_max_iter = float(cond_tol), int(cond_max_iter)
        self.cfg = cfg
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.slam_graph_create(C.byref(cfg), int(device), C.byref(h)), "slam_graph_create")
        self._h = h
        self.n_poses = 0
        self.n_edges = 0
        self.n_odom = 0
        self.n_halves = 0           # observations of the landmark map (set_observations)
        self.n_landmarks = 0
        if robust is not None:
            try:
                self.set_robust(*robust)
            except Exception:
                self.close()
                raise

    def set_robust(self, kind, param=None):
        """Robust edge weights (slam_graph_set_robust): ``kind`` is
        None / "none", or "huber" / "cauchy" (``param`` = k) or "dcs" (``param``
        = Phi).  Takes effect at the next linearisation.  Above 2048 unknowns
        use ``cond="estimate"`` (or "off") with a robust kind: the margin gate's
        det half may stay undecided on the weighted system."""
        kind = "none" if kind is None else kind
        if kind not in GRAPH_ROBUST:
            raise ValueError("robust kind must be one of %s" % (sorted(GRAPH_ROBUST),))
        if kind != "none" and param is None:
            raise ValueError("robust kind %r needs its parameter" % (kind,))
        check(self._lib.slam_graph_set_robust(self._h, GRAPH_ROBUST[kind],
                                              0.0 if param is None else float(param)),
              "slam_graph_set_robust")

    def set_precond(self, kind, segment=None):
        """Preconditioner of the PCG path (slam_graph_set_precond):
        None / "block_jacobi" (the default), "chain", or ("chain", S) with the
        segment length S in 1, 2, 4 .. 64 poses (``segment``, or 0 / None: 64).
        Takes effect at the next linearisation; no effect on the dense path."""
        if isinstance(kind, (tuple, list)):
            if len(kind) != 2 or segment is not None:
                raise ValueError("precond must be a kind or (kind, segment)")
            kind, segment = kind
        kind = "block_jacobi" if kind is None else kind
        if kind not in GRAPH_PRECOND:
            raise ValueError("precond kind must be one of %s" % (sorted(GRAPH_PRECOND),))
        check(self._lib.slam_graph_set_precond(self._h, GRAPH_PRECOND[kind],
                                               0 if segment is None else int(segment)),
              "slam_graph_set_precond")

    def precond_info(self):
        """The preconditioner the last linearisation put in force
        (slam_graph_precond_info): kind, segment (1 for block-Jacobi), and of the
        last chain factor the off-diagonal blocks it used and its bad pivots."""
        out = np.zeros(4)
        check(self._lib.slam_graph_precond_info(self._h, dptr(out)), "slam_graph_precond_info")
        names = {v: k for k, v in GRAPH_PRECOND.items()}
        return dict(kind=names[int(out[0])], segment=int(out[1]), off_diagonal_blocks=int(out[2]),
                    bad_pivots=int(out[3]))

    def apply_precond(self, r):
        """z = M^-1 r by the preconditioner in force on the last assembled system
        (slam_graph_apply_precond): ``r`` has 3 nt values in the order of
        get_system's times.  Moves nothing."""
        nt = C.c_int64(0)
        check(self._lib.slam_graph_get_system(self._h, C.byref(nt), None, None, None, None),
              "slam_graph_get_system")
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
        if len(r) != 3 * nt.value:
            raise ValueError("r must have 3 nt = %d values" % (3 * nt.value,))
        z = np.empty(len(r))
        check(self._lib.slam_graph_apply_precond(self._h, dptr(r), dptr(z)),
              "slam_graph_apply_precond")
        return z

    def chi2(self, per_edge=False):
        """Chi-square of the edge set at the current poses under the handle's
        robust kind (slam_graph_chi2): dict(chi2=sum chi2_e, cost=sum rho_e,
        max_chi2, n_low_weight=edges with w < 0.1), plus the per-edge arrays
        ``edge_chi2`` and ``edge_weight`` with ``per_edge=True``.  Moves nothing."""
        tot = np.zeros(4)
        c = np.empty(self.n_edges) if per_edge else None
        w = np.empty(self.n_edges) if per_edge else None
        check(self._lib.slam_graph_chi2(self._h, dptr(tot), dptr(c), dptr(w)), "slam_graph_chi2")
        out = dict(chi2=float(tot[0]), cost=float(tot[1]), max_chi2=float(tot[2]),
                   n_low_weight=int(tot[3]))
        if per_edge:
            out["edge_chi2"], out["edge_weight"] = c, w
        return out

    def edge_weights(self):
        """(chi2, weight) per edge as the last linearisation stored them: the
        weights the last assembled H used (slam_graph_get_edge_weights; an
        error on a handle whose last linearisation ran without a robust kind)."""
        c, w = np.empty(self.n_edges), np.empty(self.n_edges)
        check(self._lib.slam_graph_get_edge_weights(self._h, dptr(c), dptr(w)),
              "slam_graph_get_edge_weights")
        return c, w

    def set_observations(self, halves, n_landmarks):
        """The observations of the landmark map (slam_graph_set_observations;
        DESIGN 8.7): HALF_DTYPE records or rows [time, pose_id, landmark, dist,
        dir, orient], as ``pair_halves`` takes them, grouped per landmark once.
        A landmark id outside [0, n_landmarks) is ignored.  No half-edge clears
        them; ``set_poses`` with another pose count drops them."""
        rec = half_array(halves)
        check(self._lib.slam_graph_set_observations(self._h, len(rec), rec.ctypes.data_as(C.c_void_p),
                                                    int(n_landmarks)), "slam_graph_set_observations")
        self.n_halves, self.n_landmarks = len(rec), int(n_landmarks)

    def landmarks(self, per_observation=False):
        """The landmark map at the current poses (slam_graph_landmarks): (mean
        (NL, 2), cov (NL, 2, 2), count (NL,), chi2 (NL,)), and with
        ``per_observation=True`` the chi-square of every half-edge in input order
        (NaN for an ignored one).  Each landmark is the information-weighted
        fusion of its observations given the poses; the covariance does not
        contain the uncertainty of the poses.  NaN where count is 0.  Moves
        nothing."""
        nl = self.n_landmarks
        mean, cov, chi2 = np.empty((nl, 2)), np.empty((nl, 2, 2)), np.empty(nl)
        count = np.zeros(nl, dtype=np.int64)
        half = np.empty(self.n_halves) if per_observation else None
        check(self._lib.slam_graph_landmarks(self._h, dptr(mean), dptr(cov),
                                             count.ctypes.data_as(C.POINTER(C.c_int64)), dptr(chi2),
                                             dptr(half)), "slam_graph_landmarks")
        return (mean, cov, count, chi2, half) if per_observation else (mean, cov, count, chi2)

    def map_timing(self):
        """Device time of the last ``landmarks`` (slam_graph_map_timing and
        slam_graph_map_kernel_timing): the kernels' total, their number, and the
        ms of each in launch order."""
        out, ker = np.zeros(2), np.zeros(5)
        check(self._lib.slam_graph_map_timing(self._h, dptr(out)), "slam_graph_map_timing")
        check(self._lib.slam_graph_map_kernel_timing(self._h, dptr(ker)), "slam_graph_map_kernel_timing")
        return dict(ms=out[0], launches=int(out[1]), contrib_ms=ker[0], fold_ms=ker[1], finish_ms=ker[2],
                    chi2_fold_ms=ker[3], chi2_finish_ms=ker[4])

    def close(self):
        if getattr(self, "_h", None):
            self._lib.slam_graph_destroy(self._h)
            self._h = None

    __del__ = close

    def set_poses(self, poses):
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
        check(self._lib.slam_graph_set_poses(self._h, len(poses), dptr(poses)), "slam_graph_set_poses")
        if len(poses) != self.n_poses:
            self.n_halves = self.n_landmarks = 0    # the handle dropped the observations
        self.n_poses = len(poses)

    def get_poses(self):
        out = np.empty((self.n_poses, 3))
        check(self._lib.slam_graph_get_poses(self._h, dptr(out)), "slam_graph_get_poses")
        return out

    def set_edges(self, edges, odometry=None):
        """The edge set: landmark pairs, and with ``odometry`` (ODOM_DTYPE records
        or odom_array rows) the odometry edges behind them
        (slam_graph_set_edges_odom).  ``n_edges`` is the total, ``n_odom`` the
        odometry count; per-edge results are over all of them, pairs first."""
        rec = edges if (isinstance(edges, np.ndarray) and edges.dtype == EDGE_DTYPE) else edge_array(edges)
        rec = np.ascontiguousarray(rec)
        if odometry is None:
            check(self._lib.slam_graph_set_edges(self._h, len(rec), rec.ctypes.data_as(C.c_void_p)),
                  "slam_graph_set_edges")
            self.n_edges, self.n_odom = len(rec), 0
            return
        od = odometry if (isinstance(odometry, np.ndarray) and odometry.dtype == ODOM_DTYPE) \
            else odom_array(odometry)
        od = np.ascontiguousarray(od)
        check(self._lib.slam_graph_set_edges_odom(self._h, len(rec), rec.ctypes.data_as(C.c_void_p),
                                                  len(od), od.ctypes.data_as(C.c_void_p)),
              "slam_graph_set_edges_odom")
        self.n_edges, self.n_odom = len(rec) + len(od), len(od)

    def update(self):
        """updateEstPose: returns (is_calc, delta_sum, det, cond)."""
        st = np.zeros(4)
        check(self._lib.slam_graph_update(self._h, dptr(st)), "slam_graph_update")
        return bool(st[0]), float(st[1]), float(st[2]), float(st[3])

    def optimize(self, delta_sum_th=0.01, max_iter=100):
        st = np.zeros((max_iter, 4))
        n = C.c_int32(0)
        check(self._lib.slam_graph_optimize(self._h, float(delta_sum_th), int(max_iter), dptr(st),
                                            C.byref(n)), "slam_graph_optimize")
        return st[:n.value]

    def get_system(self, dense=True, blocks=False):
        nt = C.c_int64(0)
        check(self._lib.slam_graph_get_system(self._h, C.byref(nt), None, None, None, None),
              "slam_graph_get_system")
        n = 3 * nt.value
        times = np.empty(nt.value, dtype=np.int64)
        H = np.empty((n, n)) if dense else None
        b = np.empty(n)
        blk = np.empty((self.n_edges, 42)) if blocks else None
        check(self._lib.slam_graph_get_system(self._h, C.byref(nt),
                                              times.ctypes.data_as(C.POINTER(C.c_int64)),
                                              dptr(H), dptr(b), dptr(blk)), "slam_graph_get_system")
        return times, H, b, blk

    def get_bsr(self):
        """(rows, cols, vals (n_slots, 3, 3)) of the last assembled H."""
        ns = C.c_int64(0)
        check(self._lib.slam_graph_get_bsr(self._h, C.byref(ns), None, None, None), "slam_graph_get_bsr")
        rows = np.empty(ns.value, dtype=np.int64)
        cols = np.empty(ns.value, dtype=np.int64)
        vals = np.empty((ns.value, 3, 3))
        P64 = C.POINTER(C.c_int64)
        check(self._lib.slam_graph_get_bsr(self._h, C.byref(ns), rows.ctypes.data_as(P64),
                                           cols.ctypes.data_as(P64), dptr(vals)), "slam_graph_get_bsr")
        return rows, cols, vals

    def get_delta(self):
        nt = C.c_int64(0)
        check(self._lib.slam_graph_get_system(self._h, C.byref(nt), None, None, None, None),
              "slam_graph_get_system")
        out = np.empty(3 * nt.value)
        check(self._lib.slam_graph_get_delta(self._h, dptr(out)), "slam_graph_get_delta")
        return out

    def timing(self):
        out = np.zeros(5)
        check(self._lib.slam_graph_timing(self._h, dptr(out)), "slam_graph_timing")
        return dict(linearize_ms=out[0], assemble_ms=out[1], solve_ms=out[2], update_ms=out[3],
                    pcg_iterations=int(out[4]))

    def cond_info(self):
        """The last PCG-path update's condition estimate (slam_graph_cond_info)."""
        out = np.zeros(7)
        check(self._lib.slam_graph_cond_info(self._h, dptr(out)), "slam_graph_cond_info")
        return dict(iterations=int(out[0]), status=int(out[1]), lambda_min=out[2],
                    lambda_max=out[3], iterations_min=int(out[4]), iterations_max=int(out[5]),
                    ms=out[6])

    def marginals(self, times, relinearize=True, joint=False, symmetrize=True):
        """Marginal covariances of the poses at ``times`` (distinct times of the
        edge set): blocks of H^-1 (slam_graph_marginals).  ``relinearize=True``
        linearises at the current poses first, ``False`` uses the system the
        last update assembled.  Returns (is_calc, cov, info): cov is (m, 3, 3),
        the diagonal blocks, or with ``joint=True`` the whole (3m, 3m) joint
        covariance (block (a, b) = times[a] x times[b]); all NaN when is_calc is
        False.  ``symmetrize`` averages the joint matrix with its transpose on
        the host (H, and so its inverse, is symmetric only to rounding)."""
        times = np.ascontiguousarray(times, dtype=np.int64).reshape(-1)
        m = len(times)
        cov = np.empty((3 * m, 3 * m))
        out = np.zeros(6)
        check(self._lib.slam_graph_marginals(self._h, m, times.ctypes.data_as(C.POINTER(C.c_int64)),
                                             1 if relinearize else 0, dptr(cov), dptr(out)),
              "slam_graph_marginals")
        if symmetrize:
            cov = 0.5 * (cov + cov.T)
        if not joint:
            cov = np.stack([cov[3 * a:3 * a + 3, 3 * a:3 * a + 3] for a in range(m)])
        info = dict(passes=int(out[1]), iterations=int(out[2]), residual=out[3], ms=out[4],
                    cols=int(out[5]))
        return bool(out[0]), cov, info

    def set_marginal_cols(self, cols):
        """Columns per pass of the PCG path of ``marginals`` (1, 2, 4 or 8; 0:
        the default).  The result's bits do not depend on it."""
        check(self._lib.slam_graph_set_marginal_cols(self._h, int(cols)),
              "slam_graph_set_marginal_cols")

    def gate_info(self):
        """The last PCG-path update's gate (cond="margin": an estimate with
        margins, not a certificate; slam_graph_gate_info): the log-det interval,
        the cond(H) the decision used, the Ritz values, each half's decision and
        the margins the decisions held (det_margin: the factor by which the Ritz
        lambda_min may over-estimate lambda_min(H) before the det lower end
        drops below ln det_min; cond_margin: cond_max / cond)."""
        out = np.zeros(14)
        check(self._lib.slam_graph_gate_info(self._h, dptr(out)), "slam_graph_gate_info")
        return dict(decided_by="bounds" if out[0] == 1 else "dense" if out[0] == 2 else "none",
                    det_decision=int(out[1]), det=GATE_DET.get(int(out[1]), "none"),
                    cond_decision=int(out[2]), logdet_lo=out[3], logdet_hi=out[4],
                    cond=out[5], lambda_min=out[6], lambda_max=out[7], trp2=out[8],
                    n=int(out[9]), estimate_iterations=int(out[10]), ms=out[11],
                    det_margin=out[12], cond_margin=out[13],
                    cond_decided=GATE_COND.get(int(out[2]), "none"))


MEMBER_MAX_POSES = 682      # 2046 unknowns: the dense path's limit (slam_graph_set_members)


class DeviceGraphEnsemble:
    """Many pose graphs of the dense path's size on one GPU, advanced together
    with one launch per phase (slam_graph_set_members).  Takes
    DeviceGraph's keywords and composes one DeviceGraph.  Member m is bit for
    bit what a stand-alone DeviceGraph with the same keywords returns for member
    m's poses and edges alone."""

    def __init__(self, **kwargs):
        self._dev = DeviceGraph(**kwargs)
        self._lib = self._dev._lib
        self.n_members = 0
        self._pose_off = np.zeros(1, dtype=np.int64)
        self._lm_off = np.zeros(1, dtype=np.int64)
        self._od_off = np.zeros(1, dtype=np.int64)

    def set_robust(self, kind, param=None):
        """One robust kind for all members (DeviceGraph.set_robust)."""
        self._dev.set_robust(kind, param)

    def close(self):
        self._dev.close()

    def set_members(self, members):
        """``members``: a list of (poses, edges) or (poses, edges, odometry) with
        member-local times and pose ids, edges and odometry as DeviceGraph.set_edges
        takes them.  Concatenates them, offsets the indices and hands the union
        to the handle; per-member results come back in the members' own order."""
        poses, lm, od = [], [], []
        for mem in members:
            p = np.ascontiguousarray(mem[0], dtype=np.float64).reshape(-1, 3)
            e = mem[1]
            e = e if (isinstance(e, np.ndarray) and e.dtype == EDGE_DTYPE) else edge_array(e)
            o = mem[2] if len(mem) > 2 and mem[2] is not None else np.zeros(0, dtype=ODOM_DTYPE)
            o = o if (isinstance(o, np.ndarray) and o.dtype == ODOM_DTYPE) else odom_array(o)
            poses.append(p)
            lm.append(e)
            od.append(o)
        if not poses:
            raise ValueError("an ensemble needs at least one member")
        pose_off = np.concatenate([[0], np.cumsum([len(p) for p in poses])]).astype(np.int64)

        def shifted(recs):
            out = []
            for m, r in enumerate(recs):
                r = r.copy()
                for name in ("time_bfr", "pose_bfr", "time_aft", "pose_aft"):
                    r[name] += pose_off[m]
                out.append(r)
            return np.concatenate(out)

        self._dev.set_poses(np.concatenate(poses))
        check(self._lib.slam_graph_set_members(self._dev._h, len(poses),
                                               pose_off.ctypes.data_as(C.POINTER(C.c_int64))),
              "slam_graph_set_members")
        self.n_members = len(poses)
        self._pose_off = pose_off
        self._lm_off = np.concatenate([[0], np.cumsum([len(e) for e in lm])]).astype(np.int64)
        self._od_off = np.concatenate([[0], np.cumsum([len(o) for o in od])]).astype(np.int64)
        all_od = shifted(od)
        self._dev.set_edges(shifted(lm), odometry=all_od if len(all_od) else None)

    def update(self):
        """One updateEstPose of every member: (B, 4) rows (is_calc, delta_sum,
        det, cond); a zero row for a member with no edge or a single time."""
        st = np.zeros((self.n_members, 4))
        check(self._lib.slam_graph_update_members(self._dev._h, dptr(st)), "slam_graph_update_members")
        return st

    def optimize(self, delta_sum_th=0.01, max_iter=100):
        """Every member's Gauss-Newton loop; a member that has stopped is left
        alone.  Returns a list of (n_iter_m, 4) arrays."""
        st = np.zeros((self.n_members, max_iter, 4))
        n = np.zeros(self.n_members, dtype=np.int32)
        check(self._lib.slam_graph_optimize_members(self._dev._h, float(delta_sum_th), int(max_iter),
                                                    dptr(st), n.ctypes.data_as(C.POINTER(C.c_int32))),
              "slam_graph_optimize_members")
        return [st[m, :n[m]].copy() for m in range(self.n_members)]

    def get_poses(self):
        p = self._dev.get_poses()
        return [p[a:b] for a, b in zip(self._pose_off[:-1], self._pose_off[1:])]

    def _rows(self):
        """Per member the block rows of the union (the ranks of its times)."""
        nt = C.c_int64(0)
        check(self._lib.slam_graph_get_system(self._dev._h, C.byref(nt), None, None, None, None),
              "slam_graph_get_system")
        times = np.empty(nt.value, dtype=np.int64)
        check(self._lib.slam_graph_get_system(self._dev._h, C.byref(nt),
                                              times.ctypes.data_as(C.POINTER(C.c_int64)), None, None,
                                              None), "slam_graph_get_system")
        cut = np.searchsorted(times, self._pose_off)
        return times, cut

    def get_delta(self):
        """Per member the delta of its last solved update (3 per time of its edges)."""
        _, cut = self._rows()
        d = self._dev.get_delta()
        return [d[3 * a:3 * b] for a, b in zip(cut[:-1], cut[1:])]

    def get_system(self):
        """Per member (times, H, b) of its last assembled system, times
        member-local; H is the member's diagonal block of the union's
        block-sparse H (slam_graph_get_bsr), copied, not recomputed."""
        times, cut = self._rows()
        b = self._dev.get_system(dense=False)[2]
        rows, cols, vals = self._dev.get_bsr()
        out = []
        for m, (r0, r1) in enumerate(zip(cut[:-1], cut[1:])):
            n = int(r1 - r0)
            H = np.zeros((n, 3, n, 3))
            sel = (rows >= r0) & (rows < r1)
            H[rows[sel] - r0, :, cols[sel] - r0, :] = vals[sel]
            out.append((times[r0:r1] - self._pose_off[m], H.reshape(3 * n, 3 * n), b[3 * r0:3 * r1]))
        return out

    def edge_weights(self):
        """Per member (chi2, weight) of its columns in stand-alone order: its
        landmark pairs, then its odometry edges."""
        c, w = self._dev.edge_weights()
        n_lm = int(self._lm_off[-1])
        out = []
        for m in range(self.n_members):
            i = np.concatenate([np.arange(self._lm_off[m], self._lm_off[m + 1]),
                                n_lm + np.arange(self._od_off[m], self._od_off[m + 1])])
            out.append((c[i], w[i]))
        return out


GATE_DET = {1: "passed (log-det lower end, estimate with 1000x margin)",
            0: "rejected (log-det upper end, Fischer bound)", 3: "passed (dense LU det)",
            2: "rejected (dense LU det)", -1: "undecided"}
GATE_COND = {1: "passed (estimate with margin)", 0: "rejected (estimate: for certain)",
             5: "passed (converged estimate inside the margin band)",
             3: "passed (dense Lanczos cond)", 2: "rejected (dense Lanczos cond)", -1: "undecided"}


def _circle_world(n_poses, n_landmarks, rs):
    """circle_graph's world: (true poses (T,3), landmarks (NL,2), visibility
    (T,NL), noisy (distance, direction, orientation) (T,NL,3)); three arrays of
    standard normals drawn from ``rs`` in that order."""
    step = np.deg2rad(10.0)
    ang = np.arange(n_poses) * step
    truth = np.column_stack([10 * np.cos(ang), 10 * np.sin(ang),
                             np.mod(ang + np.pi / 2 + np.pi, 2 * np.pi) - np.pi])
    la = np.linspace(0, 2 * np.pi, n_landmarks, endpoint=False)
    lm = np.column_stack([14 * np.cos(la), 14 * np.sin(la)])
    # visibility and noisy (distance, direction, orientation) per pose
    d = lm[None, :, :] - truth[:, None, :2]
    psi = np.pi / 2 - truth[:, 2]
    rx = np.cos(psi)[:, None] * d[..., 0] - np.sin(psi)[:, None] * d[..., 1]
    ry = np.sin(psi)[:, None] * d[..., 0] + np.cos(psi)[:, None] * d[..., 1]
    dist = np.hypot(rx, ry)
    vis = (dist <= 15.0) & (ry >= np.abs(rx) * np.tan(np.pi / 2 - np.deg2rad(80.0)))
    bearing = np.arctan2(ry, rx)
    orient = np.repeat((np.pi / 2 - truth[:, 2])[:, None], n_landmarks, 1)   # ScanSensor :153
    obs = np.stack([dist * (1 + 0.05 * rs.standard_normal(dist.shape)),
                    bearing + np.deg2rad(2.0) * rs.standard_normal(dist.shape),
                    orient + np.deg2rad(2.0) * rs.standard_normal(dist.shape)], -1)
    obs[..., 1:] = np.mod(obs[..., 1:] + np.pi, 2 * np.pi) - np.pi
    return truth, lm, vis, obs


def circle_graph(n_poses, n_landmarks=64, loops_per_pose=3, seed=0, odom_noise=0.02):
    """Synthetic pose graph of the graph_based_slam.py form (BASELINE config 5):
    a robot circling at 10 m radius with a ScanSensor (15 m, +-80 deg,
    :899-902) among ``n_landmarks`` landmarks on a 14 m ring; one edge per
    consecutive pose pair sharing a landmark and ``loops_per_pose`` loop edges
    per pose between observations of the same landmark at other times.
    Returns (initial pose estimates (T,3), true poses (T,3), edge records)."""
    rs = np.random.RandomState(seed)
    truth, _, vis, obs = _circle_world(n_poses, n_landmarks, rs)
    seen_by = [np.flatnonzero(vis[:, j]) for j in range(n_landmarks)]
    rows = []

    def add(t1, t2, j):
        a, b = (t1, t2) if t1 < t2 else (t2, t1)
        rows.append((a, a, *obs[a, j], b, b, *obs[b, j]))

    for t in range(1, n_poses):
        common = np.flatnonzero(vis[t - 1] & vis[t])
        if len(common):
            add(t - 1, t, int(common[rs.randint(len(common))]))
        vis_t = np.flatnonzero(vis[t])
        for _ in range(loops_per_pose if len(vis_t) else 0):
            j = int(vis_t[rs.randint(len(vis_t))])
            others = seen_by[j]
            o = int(others[rs.randint(len(others))])
            if o != t:
                add(o, t, j)
    rec = np.zeros(len(rows), dtype=EDGE_DTYPE)
    r = np.array(rows, dtype=np.float64)
    rec["time_bfr"] = r[:, 0].astype(np.int64)
    rec["pose_bfr"] = r[:, 1].astype(np.int64)
    rec["obs_bfr"] = r[:, 2:5]
    rec["time_aft"] = r[:, 5].astype(np.int64)
    rec["pose_aft"] = r[:, 6].astype(np.int64)
    rec["obs_aft"] = r[:, 7:10]
    init = truth + np.cumsum(odom_noise * rs.standard_normal(truth.shape), axis=0)
    init[:, 2] = np.mod(init[:, 2] + np.pi, 2 * np.pi) - np.pi
    return init, truth, rec


def circle_graph_halves(n_poses, n_landmarks=64, seed=0, odom_noise=0.02):
    """circle_graph's world with every visible landmark a half-edge (time = pose
    id, recording order: by pose, then by landmark id).  Returns (initial pose
    estimates (T,3), true poses (T,3), HALF_DTYPE records, landmarks (NL,2))."""
    rs = np.random.RandomState(seed)
    truth, lm, vis, obs = _circle_world(n_poses, n_landmarks, rs)
    t, j = np.nonzero(vis)
    rec = np.zeros(len(t), dtype=HALF_DTYPE)
    rec["time"], rec["pose"], rec["landmark"], rec["obs"] = t, t, j, obs[t, j]
    init = truth + np.cumsum(odom_noise * rs.standard_normal(truth.shape), axis=0)
    init[:, 2] = np.mod(init[:, 2] + np.pi, 2 * np.pi) - np.pi
    return init, truth, rec, lm


def circle_graph_odometry(truth, sigma, seed):
    """Odometry edges of a circle_graph trajectory: one per
    consecutive pose pair (time = pose id = k-1 -> k), rel = relpose(truth[k-1],
    truth[k]) + sigma * standard normals of RandomState(1000 + seed), three per
    edge, drawn in order k = 1 .. T-1.  Returns ODOM_DTYPE records."""
    truth = np.asarray(truth, dtype=np.float64).reshape(-1, 3)
    sigma = np.asarray(sigma, dtype=np.float64).reshape(3)
    rs = np.random.RandomState(1000 + seed)
    rec = np.zeros(max(len(truth) - 1, 0), dtype=ODOM_DTYPE)
    for k in range(1, len(truth)):
        rec[k - 1] = (k - 1, k - 1, k, k, relpose(truth[k - 1], truth[k]) + sigma * rs.standard_normal(3),
                      sigma)
    return rec
