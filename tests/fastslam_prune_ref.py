"""NumPy restatement of landmark evidence and the removal of unsupported
landmarks on an associating FastSLAM filter -- the test oracle of
slam_fs_set_pruning (include/slam_hip.h states the same contract).

Each slot j < cnt_p of each particle carries an int32 evidence value.  The pass
runs after the map update of a step (fastslam_da_ref.FSDARef's or
fastslam2_da_ref.FS2DARef's), on every step, k = 0 included.  With cnt0_p the
count before the update, cnt_p the count after it and (x, y, th) the particle's
current pose, for every slot j < cnt_p in slot order:

  1. j >= cnt0_p (created by this update): ev = init;
  2. an observation of this update matched the slot: ev = min(ev + hit, ev_max);
  3. otherwise dx = mx - x, dy = my - y, and with c, s = cos, sin(pi/2 - th):
     rx = c dx - s dy, ry = s dx + c dy (world2robot, as fastslam_ref.observe);
     in view when dx dx + dy dy <= view_range view_range and, with an angle,
     also ry >= |rx| view_tan (view_tan = tan(pi/2 - view_angle)); a NaN
     comparison is "not in view".  In view: ev -= miss (not below INT32_MIN);
  4. slots with ev < remove_below are removed: the survivors keep their order
     and move down with mean, covariance and evidence, bit for bit.

``prune_pass`` is vectorised over particles and slots for the dtype of the
filter it acts on (float64, and np.longdouble to show that float64's rounding
decides no visibility test); ``prune_loop`` is the same pass as a plain
per-particle Python loop, which the vectorised form is checked against.
``PruneRef`` wraps a filter: its ``step`` is the parent's step, the evidence
gathered by the resampling indices, then the pass.  Per step it also returns
the smallest *visibility margin*: over the unmatched old slots,
|sqrt(dx^2 + dy^2) - view_range|, and |ry - |rx| view_tan| with an angle.
Test infrastructure only: the shipped path never imports it.
"""
from __future__ import annotations

import numpy as np

I32_MIN = int(np.iinfo(np.int32).min)


class PruneConfig:
    """The front end's keywords; ``view_tan`` is the double the handle is given."""

    def __init__(self, view_range, view_angle=None, init=1, hit=1, miss=1, ev_max=2 ** 31 - 1,
                 remove_below=0):
        self.view_range = float(view_range)
        self.use_angle = view_angle is not None
        self.view_tan = float(np.tan(np.pi / 2 - view_angle)) if self.use_angle else 0.0
        self.init, self.hit, self.miss = int(init), int(hit), int(miss)
        self.ev_max, self.remove_below = int(ev_max), int(remove_below)

    def front_end(self, view_angle=None):
        """The ``prune=`` dict of DeviceFastSLAM (the angle is not recoverable
        from its tangent bit for bit, so the caller passes it again)."""
        return dict(view_range=self.view_range, view_angle=view_angle, init=self.init, hit=self.hit,
                    miss=self.miss, ev_max=self.ev_max, remove_below=self.remove_below)


def _matched(assoc, n, cap):
    m = np.zeros((n, cap), dtype=bool)
    for a in np.asarray(assoc).reshape(-1, n):
        pm = np.flatnonzero(a >= 0)
        m[pm, a[pm]] = True
    return m


def prune_pass(ref, ev, assoc, cnt0, cfg):
    """The pass on filter ``ref`` (poses, counts and maps after the update) and
    the evidence ``ev`` [n][cap] (int32, as it stood before the update, already
    gathered): updates ``ref.cnt / mean / cov`` in place and returns
    (ev_new, info) with info = removed [n], moved (slots that changed place),
    margin (the smallest visibility margin, inf without an unmatched old slot),
    in_view [n][cap] (the decisions on the unmatched old slots) and src [n][cap]
    (the slot before the compaction that each slot below the new count holds)."""
    t, n, cap = ref.t, ref.n, ref.cap
    cnt = ref.cnt
    j = np.arange(cap)[None, :]
    live = j < cnt[:, None]
    new = live & (j >= np.asarray(cnt0)[:, None])
    old = live & ~new
    hit = old & _matched(assoc, n, cap)
    unm = old & ~hit
    dx = ref.mean[..., 0] - ref.x[:, None]
    dy = ref.mean[..., 1] - ref.y[:, None]
    vr = t(cfg.view_range)
    with np.errstate(invalid="ignore"):
        q = dx * dx + dy * dy
        in_view = q <= vr * vr
        margin = np.abs(np.sqrt(q) - vr)
        if cfg.use_angle:
            psi = t(np.pi / 2) - ref.th
            c, s = np.cos(psi)[:, None], np.sin(psi)[:, None]
            rx, ry = c * dx - s * dy, s * dx + c * dy
            lim = np.abs(rx) * t(cfg.view_tan)
            in_view = in_view & (ry >= lim)
            margin = np.minimum(margin, np.abs(ry - lim))
    in_view = in_view & unm
    e = np.asarray(ev).astype(np.int64)
    e = np.where(new, cfg.init, e)
    e = np.where(hit, np.minimum(e + cfg.hit, cfg.ev_max), e)
    e = np.where(in_view, np.maximum(e - cfg.miss, I32_MIN), e)
    keep = live & (e >= cfg.remove_below)
    order = np.argsort(~keep, axis=1, kind="stable")        # the kept slots first, in slot order
    cnt_new = keep.sum(axis=1).astype(np.int32)
    above = j >= cnt_new[:, None]
    mean = np.take_along_axis(ref.mean, order[..., None], axis=1)
    cov = np.take_along_axis(ref.cov, order[..., None], axis=1)
    mean[above], cov[above] = np.nan, np.nan
    e = np.take_along_axis(e, order, axis=1)
    e[above] = 0
    moved = int((keep & (np.cumsum(keep, axis=1) - 1 < j)).sum())
    mg = margin[unm & ~np.isnan(margin)]
    info = dict(removed=(cnt - cnt_new).astype(np.int32), moved=moved,
                margin=float(mg.min()) if mg.size else np.inf, in_view=in_view, src=order)
    ref.mean, ref.cov, ref.cnt = mean, cov, cnt_new
    return e.astype(np.int32), info


def prune_loop(ref, ev, assoc, cnt0, cfg):
    """``prune_pass`` as a plain per-particle loop (float64): updates ``ref`` in
    place and returns (ev_new, removed)."""
    n, cap = ref.n, ref.cap
    assoc = np.asarray(assoc).reshape(-1, n)
    ev_new = np.zeros((n, cap), dtype=np.int32)
    removed = np.zeros(n, dtype=np.int32)
    for p in range(n):
        x, y, th = float(ref.x[p]), float(ref.y[p]), float(ref.th[p])
        c, s = np.cos(np.pi / 2 - th), np.sin(np.pi / 2 - th)
        matched = {int(a) for a in assoc[:, p] if a >= 0}
        w = 0
        for j in range(int(ref.cnt[p])):
            e = int(ev[p, j])
            if j >= cnt0[p]:
                e = cfg.init
            elif j in matched:
                e = min(e + cfg.hit, cfg.ev_max)
            else:
                dx, dy = float(ref.mean[p, j, 0]) - x, float(ref.mean[p, j, 1]) - y
                seen = dx * dx + dy * dy <= cfg.view_range * cfg.view_range
                if cfg.use_angle:
                    rx, ry = c * dx - s * dy, s * dx + c * dy
                    seen = seen and ry >= abs(rx) * cfg.view_tan
                if seen:
                    e = max(e - cfg.miss, I32_MIN)
            if e >= cfg.remove_below:
                if w < j:
                    ref.mean[p, w], ref.cov[p, w] = ref.mean[p, j].copy(), ref.cov[p, j].copy()
                ev_new[p, w] = e
                w += 1
        removed[p] = int(ref.cnt[p]) - w
        ref.mean[p, w:], ref.cov[p, w:] = np.nan, np.nan
        ref.cnt[p] = w
    return ev_new, removed


class PruneRef:
    """An FSDARef or FS2DARef with evidence: ``step`` takes the parent's
    arguments and returns its outputs with ``removed`` [n], ``moved``,
    ``vis_margin``, ``in_view`` and ``cnt0`` (the counts the update started
    from, after the gather) added; ``ev`` [n][cap] is the evidence."""

    def __init__(self, ref, cfg):
        self.ref, self.cfg = ref, cfg
        self.ev = np.zeros((ref.n, ref.cap), dtype=np.int32)
        self.reset()

    def reset(self):
        """Every live slot at init (what turning pruning on, or set_counts, does)."""
        live = np.arange(self.ref.cap)[None, :] < self.ref.cnt[:, None]
        self.ev = np.where(live, self.cfg.init, 0).astype(np.int32)

    def snapshot(self):
        s = self.ref.snapshot()
        s["ev"] = self.ev.copy()
        return s

    def step(self, control, obs, noise, ofs=None):
        ref = self.ref
        pre = ref.cnt.copy()
        out = ref.step(control, obs, noise, ofs)
        if out["resampled"]:
            self.ev, pre = self.ev[out["idx"]], pre[out["idx"]]
        self.ev, info = prune_pass(ref, self.ev, out["assoc"], pre, self.cfg)
        out.update(removed=info["removed"], moved=info["moved"], vis_margin=info["margin"],
                   in_view=info["in_view"], src=info["src"], cnt0=pre)
        return out
