"""Landmark evidence and the removal of unsupported landmarks on the device
(slam_fs_set_pruning, DeviceFastSLAM(prune=...)) against its NumPy restatement,
tests/fastslam_prune_ref.py, on the scenario inputs of test_gpu_fastslam_assoc
("ml") and test_gpu_fastslam2_assoc ("ml_marginal").

Bars.  Precondition, on the oracle alone: the parent tests' association
precondition (float64 and longdouble associate identically from every step's
input state, the smallest decision margin is at least 1e-8); float64 and
longdouble also make identical in-view decisions and leave identical evidence;
the smallest visibility margin (|sqrt(dx^2 + dy^2) - view_range|, and
|ry - |rx| view_tan| with an angle, over the unmatched old slots) is at least
1e-8 m; the scenario removes at least one landmark and moves at least one slot.
The device must then match every evidence value, count, removal and choice
exactly.  Values hold the parent tests' bars: 1e-11 widened to 64 x the
oracle's own float64-against-longdouble spread.  A slot the update did not
touch holds the oracle's bits whether the pass moved it or not.

Evidence +1 / -1, removal below 0 throughout the scenarios.  The oracle finds
(removals / slots moved / smallest visibility margin): A, view range 7.2 m,
1,943 / 330 / 1.3e-5 m; A with an 80 degree half-angle 1,619 / 103 / 1.4e-4 m;
C (view range 11 m, 80 degrees) 11,358 / 140,363 / 2.4e-6 m, with 251,908
drops in the same run; A on "ml_marginal" 2,175 / 1,920 / 1.4e-4 m
(DESIGN 11f).
"""
import numpy as np
import pytest

from conftest import ORACLE, heavy_weights  # noqa: F401

import fastslam2_da_ref as d2
import fastslam_da_ref as da
import fastslam_prune_ref as pr
import fastslam_ref as fr
import pf_oracle as po
import test_gpu_fastslam2_assoc as t2
import test_gpu_fastslam_assoc as t1
from test_gpu_fastslam import LD, NOISE, _err_big, _err_cov, _err_mean, _rel_w, _same
from test_gpu_fastslam2 import _ties
from test_gpu_fastslam_assoc import P_NEW, SCENARIOS, _held, _load, _nan_above

pytestmark = pytest.mark.gpu

MARGIN_BAR = 1e-8
ANGLE = np.deg2rad(80.0)
RUNS = {
    # name: handle kind, the parent tests' scenario, view range, view half-angle
    "A": ("ml", "A", 7.2, None),
    "Aa": ("ml", "A", 7.2, ANGLE),
    "C": ("ml", "C", 11.0, ANGLE),
    "A2": ("ml_marginal", "A", 7.2, None),
}


def _config(run):
    _, _, vr, angle = RUNS[run]
    return pr.PruneConfig(vr, view_angle=angle, init=1, hit=1, miss=1, remove_below=0)


def _oracle(kind, n, cap, dtype=np.float64):
    kw = dict(p_new=P_NEW, noise=NOISE, ess_th=n / 2.0)
    if kind == "ml":
        return da.FSDARef(n, cap, motion="linear", dtype=dtype, **kw)
    return d2.FS2DARef(n, cap, t2._q_device(), dtype=dtype, **kw)


def _device(run, **kw):
    kind, name, vr, angle = RUNS[run]
    sc = SCENARIOS[name]
    kw.setdefault("prune", _config(run).front_end(angle))
    if kind == "ml":
        return t1._device(sc, **kw)
    return t2._device(sc["n"], sc["cap"], **kw)


def _values(kind, ref, out):
    """The step's values, in the oracle's dtype."""
    v = dict(w=ref.w.copy(), pose=np.column_stack([ref.x, ref.y, ref.th]), mean=ref.mean.copy(),
             cov=ref.cov.copy(), x_est=out["x_est"], pcov=out["cov"])
    if kind == "ml_marginal":
        v.update(mu=out["mu"], sigma=out["sigma"], L=out["L"])
    return v


def _errors(a, b, cnt, max_idx):
    xe = np.asarray(b["pose"][max_idx], dtype=np.float64)
    e = dict(w=_rel_w(a["w"], b["w"]), pose=_err_mean(a["pose"], b["pose"]),
             mean=_err_mean(_held(a["mean"], cnt), _held(b["mean"], cnt)),
             cov=_err_cov(_held(a["cov"], cnt), _held(b["cov"], cnt)),
             x_est=_err_mean(a["x_est"], xe), pcov=_err_big(a["pcov"], b["pcov"]))
    if "mu" in b:
        e.update(mu=_err_mean(a["mu"], b["mu"]), sigma=_err_cov(a["sigma"], b["sigma"]),
                 L=_err_mean(a["L"], b["L"]))
    return e


def _build(run):
    """The pruning oracle's trajectory of a run, computed once: per step the
    input state, the injected inputs, the float64 outputs, whether longdouble
    from the same input state decides identically, and the spread."""
    from concurrent.futures import ThreadPoolExecutor
    kind, name, _, _ = RUNS[run]
    sc, cfg = SCENARIOS[name], _config(run)
    n, cap = sc["n"], sc["cap"]
    lm = np.random.RandomState(3).uniform(-12, 12, (sc["nl"], 2))
    ctl, poses = fr.circle_truth(sc["steps"])
    rs = np.random.RandomState(5)
    flt = pr.PruneRef(_oracle(kind, n, cap), cfg)
    steps = []
    for pose in poses:
        _, obs = fr.observe(pose, lm, sc["rng"], NOISE, rs)
        u = rs.rand()
        inp = rs.multivariate_normal([0.0, 0.0, 0.0], t1.Q, n) if kind == "ml" else \
            rs.standard_normal((n, 3))
        pre = flt.snapshot()
        out = flt.step(ctl, obs, inp, u * (1 / n))
        ws = np.sort(flt.ref.w)
        fin = out["margin"][np.isfinite(out["margin"])]
        steps.append(dict(pre=pre, obs=obs, u=u, inp=inp, out=out, post=flt.snapshot(),
                          val=_values(kind, flt.ref, out),
                          min_margin=float(fin.min()) if fin.size else np.inf,
                          top_gap=float((ws[-1] - ws[-2]) / ws[-1])))

    def against_longdouble(s):
        ld = pr.PruneRef(_oracle(kind, n, cap, LD), cfg)
        for k in ("x", "y", "th", "w", "mean", "cov"):
            setattr(ld.ref, k, s["pre"][k].astype(LD))
        ld.ref.cnt, ld.ev = s["pre"]["cnt"].copy(), s["pre"]["ev"].copy()
        o = ld.step(ctl, s["obs"], s["inp"], s["u"] * (1 / n))
        out, post = s["out"], s["post"]
        same = bool(np.array_equal(out["assoc"], o["assoc"]) and
                    np.array_equal(post["cnt"], ld.ref.cnt) and
                    np.array_equal(out["in_view"], o["in_view"]) and
                    np.array_equal(post["ev"], ld.ev) and o["max_idx"] in _ties(s["val"]))
        if not same:
            return same, {}
        return same, _errors(s["val"], _values(kind, ld.ref, o), post["cnt"], out["max_idx"])

    spread = {}
    with ThreadPoolExecutor(max_workers=8) as pool:
        for s, (same, sp) in zip(steps, pool.map(against_longdouble, steps)):
            s["same_ld"] = same
            for q, v in sp.items():
                spread[q] = max(spread.get(q, 0.0), v)
    return dict(run=run, kind=kind, sc=sc, cfg=cfg, ctl=ctl, steps=steps, spread=spread,
                final=flt)


_CACHE = {}


def scenario(run):
    if run not in _CACHE:
        _CACHE[run] = _build(run)
    return _CACHE[run]


def _precondition(run):
    S = scenario(run)
    steps = S["steps"]
    a = np.concatenate([s["out"]["assoc"].ravel() for s in steps])
    mm = min(s["min_margin"] for s in steps)
    vm = min(s["out"]["vis_margin"] for s in steps)
    removed = sum(int(s["out"]["removed"].sum()) for s in steps)
    moved = sum(s["out"]["moved"] for s in steps)
    print(f"run {run}: {a.size} choices, {int((a == da.DROPPED).sum())} dropped, "
          f"{int((a == da.NEW).sum())} new, {removed} removed, {moved} slots moved, smallest "
          f"decision margin {mm:.3g}, smallest visibility margin {vm:.3g} m, resamplings "
          f"{sum(s['out']['resampled'] for s in steps)}, final counts "
          f"{S['final'].ref.cnt.min()}..{S['final'].ref.cnt.max()}")
    for k, s in enumerate(steps):
        assert s["same_ld"], f"step {k}: float64 and longdouble decide differently"
    assert mm >= MARGIN_BAR, f"smallest decision margin {mm:.3g} < {MARGIN_BAR}"
    assert vm >= MARGIN_BAR, f"smallest visibility margin {vm:.3g} m < {MARGIN_BAR}"
    assert removed >= 1 and moved >= 1, (removed, moved)
    if run == "C":
        assert (a == da.DROPPED).any(), "C drops and removes in the same run"
    return S


def _load_all(dev, pre):
    _load(dev, pre)                     # set_counts puts the live slots at init ...
    dev.set_evidence(pre["ev"])         # ... and this overrides


def _device_values(kind, dev, rd):
    x, y, th, w = dev.get_state()
    _, mean, cov = dev.get_maps()
    v = dict(w=w, pose=np.column_stack([x, y, th]), mean=mean, cov=cov, x_est=rd["x_est"],
             pcov=rd["cov"])
    if kind == "ml_marginal":
        v["mu"], v["sigma"], v["L"] = dev.last_proposal()
    return v


def _check_decisions(S, dev, rd, s, tag):
    out, post = s["out"], s["post"]
    assert rd["resampled"] == out["resampled"], tag
    if out["assoc"].shape[0]:
        assert np.array_equal(dev.last_assoc(), out["assoc"]), tag
    assert np.array_equal(dev.get_counts(), post["cnt"]), tag
    assert np.array_equal(dev.evidence(), post["ev"]), tag
    assert np.array_equal(dev.last_removed(), out["removed"]), tag
    assert rd["resample_next"] == out["resample_next"], tag
    T = _ties(s["val"])
    assert rd["max_idx"] == out["max_idx"] if T.size == 1 else rd["max_idx"] in T, tag


# ---------------------------------------------------------------- 1. lockstep
@pytest.mark.parametrize("run", ["A", "Aa", "C", "A2"])
def test_lockstep_against_the_oracle(run):
    S = _precondition(run)
    kind, sc, steps = S["kind"], S["sc"], S["steps"]
    n, cap = sc["n"], sc["cap"]
    bar = {k: max(1e-11, 64 * v) for k, v in S["spread"].items()}
    print(f"  float64-vs-longdouble spread {S['spread']}")
    worst = dict.fromkeys(bar, 0.0)
    moved_bits = 0
    with _device(run) as dev:
        for k, s in enumerate(steps):
            _load_all(dev, s["pre"])
            dev.set_resample_next(s["out"]["resampled"])
            rd = dev.step(S["ctl"], None, s["obs"], s["inp"], s["u"])
            out, post = s["out"], s["post"]
            _check_decisions(S, dev, rd, s, k)
            cnt = post["cnt"]
            dv = _device_values(kind, dev, rd)
            assert dev.info()["n_seen"] == cnt.max(), k
            for q, e in _errors(dv, s["val"], cnt, rd["max_idx"]).items():
                worst[q] = max(worst[q], e)
                assert e <= bar[q], f"step {k}: {q} error {e:.3g} > {bar[q]:.3g}"
            assert _nan_above(dv["mean"], cnt) and _nan_above(dv["cov"], cnt), k
            # a slot no observation matched or created came through the gather and
            # the compaction only: the oracle's bits, whether it moved or not
            touched = np.zeros((n, cap), dtype=bool)
            for a in out["assoc"]:
                pm = np.flatnonzero(a >= 0)
                touched[pm, a[pm]] = True
            src = out["src"]
            slot = np.arange(cap)[None, :]
            rest = (slot < cnt[:, None]) & (src < out["cnt0"][:, None]) & \
                ~np.take_along_axis(touched, src, axis=1)
            assert np.array_equal(dv["mean"][rest], post["mean"][rest]), k
            assert np.array_equal(dv["cov"][rest], post["cov"][rest]), k
            moved_bits += int((rest & (src != slot)).sum())
    assert moved_bits > 0
    print(f"  worst device-vs-oracle errors {worst}, bars {bar}; {moved_bits} untouched slots moved")


# ---------------------------------------------------------------- 2. free run
@pytest.mark.parametrize("run", ["A", "A2"])
def test_free_run_matches_the_oracle(run):
    S = _precondition(run)
    sc, steps = S["sc"], S["steps"]
    th = sc["n"] / 2.0
    ess_gap = min(abs(s["out"]["ess"] - th) / th for s in steps)
    top_gap = min(s["top_gap"] for s in steps)
    print(f"run {run}: min |ESS - ESS_TH| / ESS_TH {ess_gap:.3g}, min top-two gap {top_gap:.3g}")
    assert ess_gap > 1e-6
    if S["kind"] == "ml":
        assert top_gap > 1e-9
    with _device(run) as dev:
        for k, s in enumerate(steps):
            rd = dev.step(S["ctl"], None, s["obs"], s["inp"], s["u"])
            _check_decisions(S, dev, rd, s, k)
        i = rd["max_idx"]
        c = int(S["final"].ref.cnt[i])
        seen, mean, cov = dev.best_map()
        assert np.array_equal(seen, (np.arange(sc["cap"]) < c).astype(np.int32))
        assert _err_mean(mean[:c], S["final"].ref.mean[i, :c]) <= 1e-9
        assert np.isnan(mean[c:]).all() and np.isnan(cov[c:]).all()


# ------------------------------------------------------------------- 3. edges
def _edge_state(n, cap, rs):
    """Counts from 0 to cap inside every wave, poses near the origin, landmarks
    within 6 m."""
    cnt = (np.arange(n) % (cap + 1)).astype(np.int32)
    if n <= 2:
        cnt[:] = (cap, cap - 1)[:n]
    mean = rs.uniform(-6, 6, (n, cap, 2))
    cov = np.tile(np.array([0.04, 0.0, 0.04]), (n, cap, 1)) * rs.uniform(0.5, 2.0, (n, cap, 1))
    live = np.arange(cap)[None, :] < cnt[:, None]
    mean[~live], cov[~live] = np.nan, np.nan
    return dict(x=rs.normal(0.0, 0.05, n), y=rs.normal(0.0, 0.05, n),
                th=np.pi / 2 + rs.normal(0.0, 0.02, n), w=np.full(n, 1 / n), cnt=cnt, mean=mean,
                cov=cov)


EDGE_PATTERNS = ("first", "last", "every", "none", "full")


def _edge_evidence(pattern, cnt, cap):
    """+5 keeps a slot whatever the step does to it (+1 / -1), -5 removes it."""
    n = cnt.size
    slot = np.arange(cap)[None, :]
    live = slot < cnt[:, None]
    if pattern == "first":
        bad = slot == 0
    elif pattern == "last":
        bad = slot == cnt[:, None] - 1
    elif pattern == "every":
        bad = np.ones((n, cap), dtype=bool)
    elif pattern == "none":
        bad = np.zeros((n, cap), dtype=bool)
    else:                                   # a slot in the middle; the full maps are the point
        bad = slot == 3
    return np.where(live, np.where(bad, -5, 5), 0).astype(np.int32)


@pytest.mark.parametrize("n", [1, 2, 255, 257])
def test_edges_one_step_from_a_set_state(n):
    from slamhip.fastslam import DeviceFastSLAM
    cap = 8
    cfg = pr.PruneConfig(4.0, view_angle=np.deg2rad(70.0), init=1, hit=1, miss=1, remove_below=0)
    rs = np.random.RandomState(100 + n)
    seen = set()
    with DeviceFastSLAM(n, cap, noise=NOISE, q=t1.Q, association="ml", p_new=P_NEW,
                        record_assoc=True, prune=cfg.front_end(np.deg2rad(70.0))) as dev:
        for k in (0, 1, 129):
            obs = np.column_stack([rs.uniform(1.0, 7.0, k), rs.uniform(-np.pi, np.pi, k),
                                   rs.normal(0.0, 0.05, k)])
            if k:
                obs[0, 0] = 30.0            # matches no landmark (all within 6 m): new, or dropped
            for pattern in EDGE_PATTERNS:
                pre = _edge_state(n, cap, rs)
                ev = _edge_evidence(pattern, pre["cnt"], cap)
                ref = da.FSDARef(n, cap, p_new=P_NEW, noise=NOISE)
                for q in ("x", "y", "th", "w", "mean", "cov"):
                    setattr(ref, q, pre[q].copy())
                ref.cnt = pre["cnt"].copy()
                flt = pr.PruneRef(ref, cfg)
                flt.ev = ev.copy()
                noise = rs.multivariate_normal([0.0, 0.0, 0.0], t1.Q, n)
                out = flt.step((0.0, 0.0), obs, noise, None)
                fin = out["margin"][np.isfinite(out["margin"])]
                assert not fin.size or fin.min() >= MARGIN_BAR, (k, pattern, fin.min())
                assert out["vis_margin"] >= MARGIN_BAR, (k, pattern, out["vis_margin"])
                cnt1 = out["cnt0"] + (out["assoc"] == da.NEW).sum(axis=0)
                live = np.arange(cap)[None, :] < out["cnt0"][:, None]
                exp = ((ev == -5) & live).sum(axis=1)
                assert np.array_equal(out["removed"], exp), (k, pattern)
                assert np.array_equal(flt.ref.cnt, cnt1 - exp), (k, pattern)
                if pattern == "full" and k:
                    full = np.flatnonzero(out["cnt0"] == cap)
                    assert full.size and (out["assoc"][0, full] == da.DROPPED).all() and \
                        (out["removed"][full] == 1).all(), "a drop and a removal together"
                    seen.add("drop+remove")
                _load_all(dev, dict(pre, ev=ev))
                rd = dev.step((0.0, 0.0), None, obs, noise)
                tag = (n, k, pattern)
                assert not rd["resampled"], tag
                if k:
                    assert np.array_equal(dev.last_assoc(), out["assoc"]), tag
                assert np.array_equal(dev.get_counts(), flt.ref.cnt), tag
                assert np.array_equal(dev.evidence(), flt.ev), tag
                assert np.array_equal(dev.last_removed(), out["removed"]), tag
                assert dev.info()["n_seen"] == flt.ref.cnt.max(), tag
                _, mean, cov = dev.get_maps()
                assert _nan_above(mean, flt.ref.cnt) and _nan_above(cov, flt.ref.cnt), tag
                assert _err_mean(_held(mean, flt.ref.cnt), _held(ref.mean, ref.cnt)) <= 1e-11, tag
                assert _err_cov(_held(cov, flt.ref.cnt), _held(ref.cov, ref.cnt)) <= 1e-11, tag
                if k == 0:                  # nothing but the compaction touched the maps
                    assert np.array_equal(mean, ref.mean, equal_nan=True), tag
                    assert np.array_equal(cov, ref.cov, equal_nan=True), tag
    assert "drop+remove" in seen


# ------------------------------------------------------------------ 4. gather
@pytest.mark.parametrize("n", [255, 4097])
def test_resample_moves_the_evidence_bit_exactly(n):
    from slamhip.fastslam import DeviceFastSLAM
    cap, u = 33, 0.37
    rs = np.random.RandomState(n)
    w = heavy_weights(rs, n)
    w = w / np.sum(w.reshape(1, n))
    x, y, th = rs.uniform(-10, 10, n), rs.uniform(-10, 10, n), rs.uniform(-3, 3, n)
    cnt = rs.randint(0, cap + 1, n).astype(np.int32)
    mean, cov = rs.uniform(-12, 12, (n, cap, 2)), rs.uniform(0.01, 2.0, (n, cap, 3))
    ev = rs.randint(-2 ** 31, 2 ** 31 - 1, (n, cap)).astype(np.int32)
    idx = po.systematic_indices(w, u * (1 / n))
    assert (idx >= 0).all() and len(set(idx.tolist())) < n
    with DeviceFastSLAM(n, cap, noise=NOISE, association="ml", prune=dict(view_range=7.2)) as dev:
        dev.set_state(x, y, th, w)
        dev.set_maps(None, mean, cov)
        dev.set_counts(cnt)
        below0 = np.arange(cap)[None, :] < cnt[:, None]
        assert np.array_equal(dev.evidence(), below0.astype(np.int32))      # init = 1 below the count
        dev.set_evidence(ev)
        assert np.array_equal(dev.evidence(), np.where(below0, ev, 0))
        assert dev.resample(u, force=True)
        gcnt, gev = dev.get_counts(), dev.evidence()
        _, gmean, _ = dev.get_maps()
        assert not dev.last_removed().any()
    assert np.array_equal(gcnt, cnt[idx])
    below = np.arange(cap)[None, :] < gcnt[:, None]
    assert np.array_equal(gev, np.where(below, ev[idx], 0))
    assert np.array_equal(gmean[below], mean[idx][below])


# -------------------------------------------------------- 5. run against step
@pytest.mark.parametrize("run", ["A", "A2"])
def test_run_equals_steps(run):
    S = scenario(run)
    steps = S["steps"][:8]
    ctl = np.tile(S["ctl"], (len(steps), 1))
    with _device(run, seed=3) as d1, _device(run, seed=3) as d2:
        d1.load_observations([(None, s["obs"]) for s in steps])
        got = d1.run(0, ctl[:5]) + d1.run(5, ctl[5:])
        one = []
        removed = 0
        for s in steps:
            one.append(d2.step(S["ctl"], None, s["obs"]))
            removed += int(d2.last_removed().sum())
        assert removed > 0 and any(r["resampled"] for r in one)
        for k, (a, b) in enumerate(zip(got, one)):
            assert _same(a, b), k
        assert np.array_equal(d1.last_assoc(), d2.last_assoc())
        assert np.array_equal(d1.get_counts(), d2.get_counts())
        assert np.array_equal(d1.evidence(), d2.evidence())
        assert np.array_equal(d1.last_removed(), d2.last_removed())
        for a, b in zip(d1.get_state() + d1.get_maps(), d2.get_state() + d2.get_maps()):
            assert np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------ 6. off means off
@pytest.mark.parametrize("run", ["A", "A2"])
def test_off_means_off(run):
    from slamhip._lib import SLAM_ERR_ARG, SlamError
    S = scenario(run)
    steps = S["steps"]
    with _device(run) as d1, _device(run, prune=None) as d2:
        for s in steps[:6]:
            d1.step(S["ctl"], None, s["obs"], s["inp"], s["u"])
        assert d1.get_counts().max() > 0
        d1.set_pruning(None)
        for call in (d1.evidence, d1.last_removed, d2.evidence, d2.last_removed,
                     lambda: d2.set_evidence(np.zeros((d2.n, d2.nl)))):
            with pytest.raises(SlamError) as e:
                call()
            assert e.value.code == SLAM_ERR_ARG
        x, y, th, w = d1.get_state()
        _, mean, cov = d1.get_maps()
        cnt = d1.get_counts()
        for d in (d1, d2):
            d.set_state(x, y, th, w)
            d.set_maps(None, np.nan_to_num(mean), np.nan_to_num(cov))
            d.set_counts(cnt)
            d.set_resample_next(d1.resample_next)
        for k, s in enumerate(steps[6:9]):
            a = d1.step(S["ctl"], None, s["obs"], s["inp"], s["u"])
            b = d2.step(S["ctl"], None, s["obs"], s["inp"], s["u"])
            if k == 0:
                # the particle covariance is summed about the previous step's estimate,
                # which is the handle's history and not a state any accessor loads: the
                # first step's covariance agrees to rounding, and from then on (both
                # handles have made the same estimate) to the bit
                assert _err_big(a["cov"], b["cov"]) <= 1e-12
                a = dict(a, cov=b["cov"])
            diff = [q for q in a if q in b and not
                    np.array_equal(np.asarray(a[q]), np.asarray(b[q]), equal_nan=True)]
            assert _same(a, b), (k, diff, [(a[q], b[q]) for q in diff])
            assert np.array_equal(d1.last_assoc(), d2.last_assoc())
            assert np.array_equal(d1.get_counts(), d2.get_counts())
            for p, q in zip(d1.get_state() + d1.get_maps(), d2.get_state() + d2.get_maps()):
                assert np.array_equal(p, q, equal_nan=True)
        # turned on again: every live slot at init
        d1.set_pruning(**S["cfg"].front_end(RUNS[run][3]))
        live = np.arange(d1.nl)[None, :] < d1.get_counts()[:, None]
        assert np.array_equal(d1.evidence(), live.astype(np.int32))


def test_info_reports_the_shrunken_maximum():
    from slamhip.fastslam import DeviceFastSLAM
    n, cap = 300, 8
    rs = np.random.RandomState(2)
    pre = _edge_state(n, cap, rs)
    pre["cnt"][:] = 5
    pre["mean"], pre["cov"] = np.nan_to_num(pre["mean"], nan=1.0), np.nan_to_num(pre["cov"], nan=1.0)
    ev = np.full((n, cap), 5, dtype=np.int32)
    ev[:, 1], ev[:, 4] = -5, -5
    with DeviceFastSLAM(n, cap, noise=NOISE, association="ml",
                        prune=dict(view_range=1e-3)) as dev:
        _load_all(dev, dict(pre, ev=ev))
        assert dev.info()["n_seen"] == 5
        dev.step((0.0, 0.0), None, np.zeros((0, 3)), np.zeros((n, 3)))
        assert dev.info()["n_seen"] == 3 and (dev.get_counts() == 3).all()
        assert (dev.last_removed() == 2).all()
        seen, mean, _ = dev.get_maps()
        assert np.array_equal(seen, (np.arange(cap) < 3).astype(np.int32))
        assert np.array_equal(mean[:, :3], pre["mean"][:, [0, 2, 3]])
        assert np.array_equal(dev.evidence()[:, :3], np.full((n, 3), 5))
        # the update walk and the gather now stop at 3: a forced resample keeps the state
        assert dev.resample(0.5, force=True)
        assert (dev.get_counts() == 3).all() and np.array_equal(dev.evidence()[:, :3], np.full((n, 3), 5))


# ------------------------------------------------------------- 7. front end
def test_frontend_prunes_and_best_map_is_the_compacted_map():
    from conftest import PKG  # noqa: F401
    from fast_slam import FastSLAM
    n, cap, nsteps = 2048, 24, 20
    lm = np.random.RandomState(3).uniform(-12, 12, (40, 2))
    ctl, poses = fr.circle_truth(nsteps)
    rs = np.random.RandomState(11)
    removed = 0
    with FastSLAM(n, cap, association="ml", p_new=P_NEW, q=t1.Q, noise=NOISE,
                  ess_threshold=n / 2.0, seed=1, prune=dict(view_range=7.2)) as slam:
        for pose in poses:
            _, obs = fr.observe(pose, lm, 9.0, NOISE, rs)
            est, cov, (seen, mean, mcov) = slam.step(ctl, (None, obs))
            removed += int(slam.dev.last_removed().sum())
        seen, mean, mcov = slam.best_map()
        c = int(slam.dev.get_counts()[slam.last["max_idx"]])
        ev = slam.dev.evidence()[slam.last["max_idx"]]
    assert removed > 0
    assert c >= 1 and np.array_equal(seen, (np.arange(cap) < c).astype(np.int32))
    assert np.isfinite(mean[:c]).all() and np.isnan(mean[c:]).all()
    assert (ev[:c] >= 0).all() and (ev[c:] == 0).all()
    with pytest.raises(ValueError, match="prune"):
        FastSLAM(n, 7, prune=dict(view_range=7.2))
    with FastSLAM(64, 7) as known:
        with pytest.raises(ValueError, match="association"):
            known.dev.set_pruning(7.2)
