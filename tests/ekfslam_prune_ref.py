"""NumPy restatement of landmark evidence and the removal of landmarks from an
associating EKF-SLAM filter -- the test oracle of slam_ekfslam_set_pruning and
slam_ekfslam_remove (include/slam_hip.h states the same contract).  It builds on
tests/ekfslam_da_ref.py (the step) and shares fastslam_prune_ref's
configuration: both estimators take the same one.

The pass runs after ``ekfslam_da_ref.observe``.  With count0 the count at
entry, count the count after the initialisation and (x, y, th) the posterior
pose, for every slot j < count in slot order:

  1. j >= count0: ev = init;
  2. matched in this call: ev = min(ev + hit, ev_max);
  3. otherwise the in-view test of fastslam_prune_ref on the slot's mean
     (range, and the fan with an angle; a NaN comparison is "not in view"):
     in view, ev -= miss (not below INT32_MIN);
  4. slots with ev < remove_below are removed: with ``keep`` the survivors in
     order and idx = [0, 1, 2] + [3 + 3 j + a for j in keep, a in 0..2],
     mu' = mu[idx], P' = P[idx][:, idx], ev' = ev[keep], and zero beyond.

``prune_pass`` is vectorised over the slots for a dtype parameter (float64, and
np.longdouble to show that float64's rounding decides no visibility test);
``prune_loop`` is the same pass as a plain per-slot loop that deletes one slot
at a time, which the vectorised form is checked against.  ``PruneRun`` is
ekfslam_da_ref.Run with evidence carried through the chain.  The *visibility
margin* of a step is fastslam_prune_ref's: over the unmatched old slots,
|sqrt(dx^2 + dy^2) - view_range|, and |ry - |rx| view_tan| with an angle.
Test infrastructure only: the shipped path never imports it.
"""
from __future__ import annotations

import functools

import numpy as np

import ekfslam_da_ref as dr
from fastslam_prune_ref import I32_MIN, PruneConfig  # noqa: F401

LD = dr.LD


def gather_index(keep):
    """idx of the contract: the robot's three rows, then the kept slots' rows."""
    keep = np.asarray(keep, dtype=np.int64)
    return np.r_[0:3, (3 + 3 * keep[:, None] + np.arange(3)).ravel()].astype(np.int64)


def remove_slots(mu, P, keep):
    """(mu', P') full size with a zero tail: the ``np.ix_`` gather of the contract."""
    idx = gather_index(keep)
    mu_n, P_n = np.zeros_like(mu), np.zeros_like(P)
    mu_n[:idx.size] = mu[idx]
    P_n[:idx.size, :idx.size] = P[np.ix_(idx, idx)]
    return mu_n, P_n


def prune_pass(mu, P, count, count0, assoc, ev, cfg, t=np.float64):
    """The pass on the state after the update and initialisation (mu, P full
    size n = 3 + 3 cap, count) with the evidence ``ev`` [cap] as it stood
    before the call.  Returns a dict: mu, P (dtype t, full size, zero tail),
    count, ev [cap] (0 at and above the count), removed, moved (surviving slots
    that changed place), first (first removed slot, -1), keep (surviving old
    slots), in_view [cap] (the decisions on the unmatched old slots) and margin
    (the smallest visibility margin, inf without an unmatched old slot)."""
    mu, P = np.asarray(mu).astype(t), np.asarray(P).astype(t)
    cap = (mu.size - 3) // 3
    j = np.arange(cap)
    live = j < count
    new = live & (j >= count0)
    old = live & ~new
    hit = np.zeros(cap, dtype=bool)
    a = np.asarray(assoc, dtype=np.int64).ravel()
    hit[a[a >= 0]] = True
    hit &= old
    unm = old & ~hit
    x, y, th = mu[:3]
    L = mu[3:].reshape(cap, 3)
    dx, dy = L[:, 0] - x, L[:, 1] - y
    vr = t(cfg.view_range)
    with np.errstate(invalid="ignore"):
        q = dx * dx + dy * dy
        in_view = q <= vr * vr
        margin = np.abs(np.sqrt(q) - vr)
        if cfg.use_angle:
            psi = t(np.pi / 2) - th
            c, s = np.cos(psi), np.sin(psi)
            rx, ry = c * dx - s * dy, s * dx + c * dy
            lim = np.abs(rx) * t(cfg.view_tan)
            in_view = in_view & (ry >= lim)
            margin = np.minimum(margin, np.abs(ry - lim))
    in_view = in_view & unm
    e = np.asarray(ev).astype(np.int64)
    e = np.where(new, cfg.init, e)
    e = np.where(hit, np.minimum(e + cfg.hit, cfg.ev_max), e)
    e = np.where(in_view, np.maximum(e - cfg.miss, I32_MIN), e)
    keep_mask = live & (e >= cfg.remove_below)
    keep = np.flatnonzero(keep_mask)
    gone = np.flatnonzero(live & ~keep_mask)
    mu_n, P_n = remove_slots(mu, P, keep)
    ev_n = np.zeros(cap, dtype=np.int32)
    ev_n[:keep.size] = e[keep]
    mg = margin[unm & ~np.isnan(margin)]
    return dict(mu=mu_n, P=P_n, count=int(keep.size), ev=ev_n, removed=int(gone.size),
                moved=int((keep != np.arange(keep.size)).sum()),
                first=int(gone[0]) if gone.size else -1, keep=keep, in_view=in_view,
                margin=float(mg.min()) if mg.size else np.inf)


def prune_loop(mu, P, count, count0, assoc, ev, cfg):
    """``prune_pass`` as a plain per-slot loop (float64): the evidence slot by
    slot, then the removed slots deleted one at a time from the back.  Returns
    (mu, P, count, ev, removed)."""
    mu, P = np.array(mu, dtype=np.float64), np.array(P, dtype=np.float64)
    n, cap = mu.size, (mu.size - 3) // 3
    x, y, th = (float(v) for v in mu[:3])
    c, s = np.cos(np.pi / 2 - th), np.sin(np.pi / 2 - th)
    matched = {int(a) for a in np.asarray(assoc).ravel() if a >= 0}
    evs, gone = [], []
    for j in range(count):
        e = int(ev[j])
        if j >= count0:
            e = cfg.init
        elif j in matched:
            e = min(e + cfg.hit, cfg.ev_max)
        else:
            dx, dy = float(mu[3 + 3 * j]) - x, float(mu[4 + 3 * j]) - y
            seen = dx * dx + dy * dy <= cfg.view_range * cfg.view_range
            if cfg.use_angle:
                rx, ry = c * dx - s * dy, s * dx + c * dy
                seen = seen and ry >= abs(rx) * cfg.view_tan
            if seen:
                e = max(e - cfg.miss, I32_MIN)
        if e >= cfg.remove_below:
            evs.append(e)
        else:
            gone.append(j)
    for j in reversed(gone):
        rows = [3 + 3 * j, 4 + 3 * j, 5 + 3 * j]
        mu = np.delete(mu, rows)
        P = np.delete(np.delete(P, rows, axis=0), rows, axis=1)
    mu_n, P_n = np.zeros(n), np.zeros((n, n))
    mu_n[:mu.size], P_n[:mu.size, :mu.size] = mu, P
    ev_n = np.zeros(cap, dtype=np.int32)
    ev_n[:len(evs)] = evs
    return mu_n, P_n, count - len(gone), ev_n, len(gone)


def observe(mu, P, count, cap, obs, log_p_new, ev, cfg, noise=dr.NOISE, t=np.float64):
    """ekfslam_da_ref.observe, then the pass.  The dict of the step with the
    pass's entries; ``mu``, ``P``, ``count`` are the state after the pass,
    ``count_mid`` the count before it."""
    r = dr.observe(mu, P, count, cap, obs, log_p_new, noise, t)
    p = prune_pass(r["mu"], r["P"], r["count"], count, r["assoc"], ev, cfg, t)
    r.update(count_mid=r["count"], margin_da=r["margin"])     # ``margin`` becomes the visibility margin
    r.update(p)
    return r


# ------------------------------------------------------------------ worlds
#        base world of ekfslam_da_ref.make_scans (seed, landmarks, view, cap, p_new, steps),
#        clutter (every, n_cl), the rule's view range and half-angle
WORLDS = {"D": ((3, 20, 9.0, 32, 0.1, 100), (4, 1), 7.2, None),
          "Da": ((3, 20, 9.0, 32, 0.1, 100), (4, 1), 7.2, np.deg2rad(80.0)),
          "E": ((5, 240, 6.0, 192, 0.1, 60), (2, 2), 4.8, None)}
RULE = dict(init=1, hit=1, miss=1, ev_max=4, remove_below=0)


def clutter_scans(scans, view, every, n_cl):
    """make_scans' scans with n_cl false detections appended on the steps with
    i % every == 1, drawn from RandomState(11): ranges uniform(2, 0.7 view),
    bearings and orientations uniform(-pi, pi).  A scan stays within MAX_OBS:
    true detections give way."""
    rs = np.random.RandomState(11)
    out = []
    for i, z in enumerate(scans):
        if i % every == 1:
            cl = np.column_stack([rs.uniform(2.0, 0.7 * view, n_cl), rs.uniform(-np.pi, np.pi, n_cl),
                                  rs.uniform(-np.pi, np.pi, n_cl)])
            z = np.vstack([z[:dr.MAX_OBS - n_cl], cl])
        out.append(z)
    return out


class PruneRun:
    """A clutter world run like ekfslam_da_ref.Run, evidence carried along:
    ``f64`` the float64 chain on its own state (per step the predicted input
    state, the evidence at entry and the step's dict), ``ld`` the long-double
    step from each of the float64 chain's inputs, ``ld_free`` the long-double
    chain on its own state with ``free_spread``, and ``plain`` the final count
    and the dropped observations of the same scans without pruning."""

    def __init__(self, name, cap=None, free=True):
        (seed, n_lm, view, cap0, p_new, steps), (every, n_cl), pview, angle = WORLDS[name]
        self.cap, self.p_new = cap or cap0, p_new
        self.log_p_new = float(np.log(p_new))
        self.angle = angle
        self.cfg = PruneConfig(pview, view_angle=angle, **RULE)
        self.lm, scans, self.ids = dr.make_scans(seed, n_lm, view, steps)
        self.scans = clutter_scans(scans, view, every, n_cl)
        self.seen = len(set(np.concatenate(self.ids).tolist()))
        cap = self.cap
        mu, P = dr.empty_state(cap)
        count, ev = 0, np.zeros(cap, dtype=np.int32)
        self.f64, self.ld = [], []
        for z in self.scans:
            mu_p, P_p = dr.predict(mu, P, count, dr.CONTROL)
            r = observe(mu_p, P_p, count, cap, z, self.log_p_new, ev, self.cfg)
            self.f64.append(dict(mu_p=mu_p, P_p=P_p, count0=count, ev0=ev, obs=z, **r))
            self.ld.append(observe(mu_p, P_p, count, cap, z, self.log_p_new, ev, self.cfg, t=LD))
            mu, P, count, ev = r["mu"], r["P"], r["count"], r["ev"]
        # the same scans without removal
        mu, P = dr.empty_state(cap)
        count = dropped = 0
        for z in self.scans:
            mu_p, P_p = dr.predict(mu, P, count, dr.CONTROL)
            r = dr.observe(mu_p, P_p, count, cap, z, self.log_p_new)
            dropped += int((r["assoc"] == dr.DROPPED).sum())
            mu, P, count = r["mu"], r["P"], r["count"]
        self.plain = dict(count=count, dropped=dropped)
        if free:
            mu, P = dr.empty_state(cap)
            count, ev = 0, np.zeros(cap, dtype=np.int32)
            sp_P = sp_mu = 0.0
            self.free_same = True
            for z, f in zip(self.scans, self.f64):
                mu_p, P_p = dr.predict(mu, P, count, dr.CONTROL)
                r = observe(mu_p, P_p, count, cap, z, self.log_p_new, ev, self.cfg, t=LD)
                self.free_same &= bool(np.array_equal(r["assoc"], f["assoc"]) and
                                       r["count"] == f["count"] and np.array_equal(r["ev"], f["ev"]))
                if r["count"] == f["count"]:
                    sp_P = max(sp_P, float(np.abs(r["P"] - f["P"]).max() / np.abs(f["P"]).max()))
                    sp_mu = max(sp_mu, float(np.abs(r["mu"] - f["mu"]).max()))
                mu, P = r["mu"].astype(np.float64), r["P"].astype(np.float64)
                count, ev = r["count"], r["ev"]
            self.ld_free = dict(mu=r["mu"], P=r["P"], count=count)
            self.free_spread = (sp_P, sp_mu)

    @property
    def decisions(self):
        return int(sum(len(z) for z in self.scans))

    @property
    def final_count(self):
        return self.f64[-1]["count"]

    def totals(self):
        """(removed, moved, dropped) over the float64 chain."""
        return (sum(s["removed"] for s in self.f64), sum(s["moved"] for s in self.f64),
                sum(int((s["assoc"] == dr.DROPPED).sum()) for s in self.f64))

    def precondition(self):
        """(the association decisions, the count, the in-view decisions and
        the evidence identical in float64 and long double from every step's
        input, smallest finite decision margin over both, smallest visibility
        margin over both)."""
        same = all(np.array_equal(a["assoc"], b["assoc"]) and a["count_mid"] == b["count_mid"] and
                   a["count"] == b["count"] and np.array_equal(a["in_view"], b["in_view"]) and
                   np.array_equal(a["ev"], b["ev"]) and np.array_equal(a["keep"], b["keep"])
                   for a, b in zip(self.f64, self.ld))
        mg = np.concatenate([s["margin_da"] for s in self.f64 + self.ld])
        mg = mg[np.isfinite(mg)]
        vis = min(s["margin"] for s in self.f64 + self.ld)
        return same, float(mg.min()) if mg.size else np.inf, float(vis)


@functools.lru_cache(maxsize=None)
def run(name, cap=None, free=True):
    return PruneRun(name, cap, free)
