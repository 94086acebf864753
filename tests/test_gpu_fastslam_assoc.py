"""FastSLAM with per-particle maximum-likelihood association on the device
(slam_fs_create_assoc, slamhip.fastslam association="ml") against its NumPy
restatement, tests/fastslam_da_ref.py.

Bars.  Precondition, on the oracle alone and before the device is touched:
from every step's input state float64 and longdouble make identical
associations, and the smallest finite decision margin is at least 1e-8 (far
above fp64 rounding of a score) -- the device must then match every
association and count exactly.  Lockstep values: test_gpu_fastslam.py's
measures and bar, 1e-11 widened to 64 x the oracle's own float64-against-
longdouble spread per scenario.  Free run: identical decisions, argmax,
associations and counts, x_est and the best map to 1e-9, after the oracle alone
has shown that no resample decision or argmax is within rounding.  The
resampling stage and run-against-step are bit-exact.

The decision margin is |l_best - log_p_new|, and l_best - l_second as well
where the best candidate is taken (below log_p_new the outcome does not depend
on which candidate is best); the smallest are A 2.6e-6, B 1.9e-5, C 1.6e-6,
D 5.9e-7.  Measured on an MI355X, weights / means / covariances: the oracle's
spread A 7.2e-14 / 3.0e-15 / 1.8e-15, B 6.7e-14 / 6.9e-16 / 1.3e-15, C 1.0e-13
/ 4.4e-15 / 1.8e-15, D 3.9e-12 / 4.4e-15 / 2.0e-15; the device's worst errors
A 1.5e-14 / 1.8e-15 / 5.7e-16, B 8.9e-15 / 8.2e-16 / 2.7e-16, C 2.8e-14 /
1.9e-15 / 5.6e-16, D 1.1e-13 / 5.1e-15 / 0.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ORACLE, heavy_weights  # noqa: F401

import fastslam_da_ref as da
import fastslam_ref as fr
import pf_oracle as po
from test_gpu_fastslam import NOISE, Q, LD, _rel_w, _err_mean, _err_cov, _err_big, _same

pytestmark = pytest.mark.gpu

P_NEW = 0.1
SCENARIOS = {
    # name: NP, landmarks in the world, sensor range, steps, capacity
    "A": dict(n=1000, nl=40, rng=9.0, steps=24, cap=24),
    "B": dict(n=1000, nl=40, rng=9.0, steps=24, cap=6),       # A with a map that is full early
    "C": dict(n=4099, nl=40, rng=14.0, steps=16, cap=32),
    "D": dict(n=513, nl=300, rng=np.inf, steps=2, cap=64),    # k = 300: three LDS passes, overflow
}
MARGIN_BAR = 1e-8


def _held(a, cnt):
    """[n][cap][c] -> the rows below each particle's count, flattened."""
    m = np.arange(a.shape[1])[None, :] < cnt[:, None]
    return a[m]


def _build(name):
    """The oracle's trajectory of a scenario, computed once: per step the input
    state, the injected inputs, the float64 outputs, whether longdouble from the
    same input state associates identically, and the float64-against-longdouble
    spread."""
    sc = SCENARIOS[name]
    n, cap = sc["n"], sc["cap"]
    lm = np.random.RandomState(3).uniform(-12, 12, (sc["nl"], 2))
    ctl, poses = fr.circle_truth(sc["steps"])
    rs = np.random.RandomState(5)
    kw = dict(p_new=P_NEW, motion="linear", noise=NOISE, ess_th=n / 2.0)
    ref = da.FSDARef(n, cap, **kw)
    steps = []
    for pose in poses:
        _, obs = fr.observe(pose, lm, sc["rng"], NOISE, rs)
        u = rs.rand()
        noise = rs.multivariate_normal([0.0, 0.0, 0.0], Q, n)
        pre = ref.snapshot()
        out = ref.step(ctl, obs, noise, u * (1 / n))
        ws = np.sort(ref.w)
        fin = out["margin"][np.isfinite(out["margin"])]
        steps.append(dict(pre=pre, obs=obs, u=u, noise=noise, out=out, post=ref.snapshot(),
                          min_margin=float(fin.min()) if fin.size else np.inf,
                          top_gap=float((ws[-1] - ws[-2]) / ws[-1])))

    def against_longdouble(s):
        """One step again in longdouble from the float64 input state (the steps
        are independent, and NumPy's longdouble loops release the GIL)."""
        ld = da.FSDARef(n, cap, dtype=LD, **kw)
        for k in ("x", "y", "th", "w", "mean", "cov"):
            setattr(ld, k, s["pre"][k].astype(LD))
        ld.cnt = s["pre"]["cnt"].copy()
        out_ld = ld.step(ctl, s["obs"], s["noise"], s["u"] * (1 / n))
        out, post = s["out"], s["post"]
        cnt = post["cnt"]
        same = bool(np.array_equal(out["assoc"], out_ld["assoc"]) and np.array_equal(cnt, ld.cnt)
                    and out["max_idx"] == out_ld["max_idx"])
        if not same:
            return same, {}
        return same, dict(w=_rel_w(post["w"], ld.w),
                          mean=_err_mean(_held(post["mean"], cnt), _held(ld.mean, cnt)),
                          cov=_err_cov(_held(post["cov"], cnt), _held(ld.cov, cnt)),
                          x_est=_err_mean(out["x_est"], out_ld["x_est"]),
                          pcov=_err_big(out["cov"], out_ld["cov"]))

    spread = dict(w=0.0, mean=0.0, cov=0.0, x_est=0.0, pcov=0.0)
    with ThreadPoolExecutor(max_workers=8) as pool:
        for s, (same, sp) in zip(steps, pool.map(against_longdouble, steps)):
            s["same_ld"] = same
            for q, v in sp.items():
                spread[q] = max(spread[q], v)
    return dict(sc=sc, ctl=ctl, steps=steps, spread=spread, final=ref, kw=kw, lm=lm, poses=poses)


_CACHE = {}


def scenario(name):
    if name not in _CACHE:
        _CACHE[name] = _build(name)
    return _CACHE[name]


def _precondition(name):
    """On the oracle alone: every decision is decided well above rounding."""
    S = scenario(name)
    steps = S["steps"]
    a = np.concatenate([s["out"]["assoc"].ravel() for s in steps])
    mm = min(s["min_margin"] for s in steps)
    disagree = sum(int((s["out"]["assoc"] != s["out"]["assoc"][:, :1]).any(axis=1).sum()) for s in steps)
    print(f"scenario {name}: {a.size} decisions, {int((a == da.DROPPED).sum())} dropped, "
          f"{int((a == da.NEW).sum())} new, smallest margin {mm:.3g}, "
          f"resamplings {sum(s['out']['resampled'] for s in steps)}, "
          f"final counts {S['final'].cnt.min()}..{S['final'].cnt.max()}, "
          f"observations the particles disagree about {disagree}")
    for k, s in enumerate(steps):
        assert s["same_ld"], f"step {k}: float64 and longdouble associate differently"
    assert mm >= MARGIN_BAR, f"smallest decision margin {mm:.3g} < {MARGIN_BAR}"
    return S


def _device(sc, **kw):
    from slamhip.fastslam import DeviceFastSLAM
    return DeviceFastSLAM(sc["n"], sc["cap"], motion="linear", noise=NOISE, q=Q,
                          ess_threshold=sc["n"] / 2.0, association="ml", p_new=P_NEW,
                          record_assoc=True, **kw)


def _load(dev, pre):
    dev.set_state(pre["x"], pre["y"], pre["th"], pre["w"])
    dev.set_maps(None, np.nan_to_num(pre["mean"]), np.nan_to_num(pre["cov"]))
    dev.set_counts(pre["cnt"])


def _nan_above(a, cnt):
    m = np.arange(a.shape[1])[None, :] >= cnt[:, None]
    return bool(np.isnan(a[m]).all())


# ---------------------------------------------------------------- 1. lockstep
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_lockstep_against_the_oracle(name):
    S = _precondition(name)
    sc, steps = S["sc"], S["steps"]
    bar = {k: max(1e-11, 64 * v) for k, v in S["spread"].items()}
    print(f"  float64-vs-longdouble spread {S['spread']}")
    print(f"  k per step {[len(s['obs']) for s in steps]}")
    if name == "B":
        assert any((s["out"]["assoc"] == da.DROPPED).any() for s in steps[:8]), "full early"
    if name == "D":
        assert all(len(s["obs"]) == 300 for s in steps)
        assert (steps[0]["out"]["assoc"] == da.DROPPED).any(), "overflow from the first step"
    worst = dict.fromkeys(bar, 0.0)
    with _device(sc) as dev:
        assert dev.info() == dict(n_particles=sc["n"], n_landmarks=sc["cap"], n_seen=0)
        for k, s in enumerate(steps):
            _load(dev, s["pre"])
            dev.set_resample_next(s["out"]["resampled"])
            rd = dev.step(S["ctl"], None, s["obs"], s["noise"], s["u"])
            ro, post = s["out"], s["post"]
            assert rd["resampled"] == ro["resampled"], k
            assert np.array_equal(dev.last_assoc(), ro["assoc"]), k
            cnt = dev.get_counts()
            assert np.array_equal(cnt, post["cnt"]), k
            assert rd["max_idx"] == ro["max_idx"], k
            assert rd["resample_next"] == ro["resample_next"], k
            x, y, th, w = dev.get_state()
            seen, mean, cov = dev.get_maps()
            assert np.array_equal(seen, (np.arange(sc["cap"]) < cnt.max()).astype(np.int32)), k
            assert dev.info()["n_seen"] == cnt.max()
            err = dict(w=_rel_w(w, post["w"]),
                       mean=_err_mean(_held(mean, cnt), _held(post["mean"], cnt)),
                       cov=_err_cov(_held(cov, cnt), _held(post["cov"], cnt)),
                       x_est=_err_mean(rd["x_est"], ro["x_est"]),
                       pcov=_err_big(rd["cov"], ro["cov"]))
            for q, e in err.items():
                worst[q] = max(worst[q], e)
                assert e <= bar[q], f"step {k}: {q} error {e:.3g} > {bar[q]:.3g}"
            assert _nan_above(mean, cnt) and _nan_above(cov, cnt), k
            # slots no observation matched or created: untouched but for the gather
            touched = np.zeros((sc["n"], sc["cap"]), dtype=bool)
            a = ro["assoc"]
            for q in range(a.shape[0]):
                pm = np.flatnonzero(a[q] >= 0)
                touched[pm, a[q, pm]] = True
            base = s["pre"]["cnt"][ro["idx"]] if ro["resampled"] else s["pre"]["cnt"]
            rest = ~touched & (np.arange(sc["cap"])[None, :] < base[:, None])
            assert np.array_equal(mean[rest], post["mean"][rest]), k
            assert np.array_equal(cov[rest], post["cov"][rest]), k
    print(f"  worst device-vs-oracle errors {worst}, bars {bar}")


# ---------------------------------------------------------------- 2. free run
@pytest.mark.parametrize("name", ["A", "C"])
def test_free_run_matches_the_oracle(name):
    S = _precondition(name)
    sc, steps = S["sc"], S["steps"]
    th = sc["n"] / 2.0
    ess_gap = min(abs(s["out"]["ess"] - th) / th for s in steps)
    top_gap = min(s["top_gap"] for s in steps)
    print(f"scenario {name}: min |ESS - ESS_TH| / ESS_TH {ess_gap:.3g}, min top-two gap {top_gap:.3g}")
    assert ess_gap > 1e-6
    assert top_gap > 1e-9
    with _device(sc) as dev:
        for k, s in enumerate(steps):
            rd = dev.step(S["ctl"], None, s["obs"], s["noise"], s["u"])
            assert rd["resampled"] == s["out"]["resampled"], k
            assert rd["max_idx"] == s["out"]["max_idx"], k
            assert np.array_equal(dev.last_assoc(), s["out"]["assoc"]), k
            assert np.array_equal(dev.get_counts(), s["post"]["cnt"]), k
            assert np.allclose(rd["x_est"], s["out"]["x_est"], rtol=1e-9, atol=0), k
        seen, mean, cov = dev.best_map()
        ref = S["final"]
        i = steps[-1]["out"]["max_idx"]
        c = int(ref.cnt[i])
        assert np.array_equal(seen, (np.arange(sc["cap"]) < c).astype(np.int32))
        assert _err_mean(mean[:c], ref.mean[i, :c]) <= 1e-9
        assert _err_cov(cov[:c], ref.cov[i, :c]) <= 1e-9
        assert np.isnan(mean[c:]).all() and np.isnan(cov[c:]).all()


# ------------------------------------------------- 3. resample stage, bit-exact
@pytest.mark.parametrize("n", [1, 255, 4097, 65539])
def test_resample_stage_is_bit_exact(n):
    from slamhip.fastslam import DeviceFastSLAM
    cap, u = 33, 0.37
    rs = np.random.RandomState(n)
    w = heavy_weights(rs, n)
    w = w / np.sum(w.reshape(1, n))
    x, y, th = rs.uniform(-10, 10, n), rs.uniform(-10, 10, n), rs.uniform(-3, 3, n)
    cnt = rs.randint(0, cap + 1, n).astype(np.int32)
    mean, cov = rs.uniform(-12, 12, (n, cap, 2)), rs.uniform(0.01, 2.0, (n, cap, 3))
    idx = po.systematic_indices(w, u * (1 / n))
    assert (idx >= 0).all()
    with DeviceFastSLAM(n, cap, noise=NOISE, association="ml") as dev:
        dev.set_state(x, y, th, w)
        dev.set_maps(None, mean, cov)
        dev.set_counts(cnt)
        assert dev.resample(u, force=True)
        gx, gy, gth, gw = dev.get_state()
        gcnt = dev.get_counts()
        gseen, gmean, gcov = dev.get_maps()
        m1 = dev.get_map(n - 1)
    assert np.array_equal(gx, x[idx]) and np.array_equal(gy, y[idx]) and np.array_equal(gth, th[idx])
    assert np.array_equal(gw, np.full(n, 1 / n))
    assert np.array_equal(gcnt, cnt[idx])
    below = np.arange(cap)[None, :] < gcnt[:, None]
    assert np.array_equal(gmean[below], mean[idx][below])
    assert np.array_equal(gcov[below], cov[idx][below])
    assert np.isnan(gmean[~below]).all() and np.isnan(gcov[~below]).all()
    assert np.array_equal(gseen, (np.arange(cap) < gcnt.max()).astype(np.int32))
    assert np.array_equal(m1[0], (np.arange(cap) < gcnt[-1]).astype(np.int32))
    assert np.array_equal(m1[1], gmean[-1], equal_nan=True)
    assert np.array_equal(m1[2], gcov[-1], equal_nan=True)


# -------------------------------------------------------- 4. multi-step run
def test_run_equals_steps_and_argument_rules():
    from slamhip._lib import SLAM_ERR_ARG, SlamError
    from slamhip.fastslam import DeviceFastSLAM
    S = scenario("A")
    sc, steps = S["sc"], S["steps"][:8]
    ctl = np.tile(S["ctl"], (len(steps), 1))
    with _device(sc, seed=3) as d1, _device(sc, seed=3) as d2:
        d1.load_observations([(None, s["obs"]) for s in steps])
        run = d1.run(0, ctl[:5]) + d1.run(5, ctl[5:])
        one = [d2.step(S["ctl"], None, s["obs"]) for s in steps]
        assert any(r["resampled"] for r in one)
        for k, (a, b) in enumerate(zip(run, one)):
            assert _same(a, b), k
        assert np.array_equal(d1.last_assoc(), d2.last_assoc())
        assert np.array_equal(d1.get_counts(), d2.get_counts())
        assert d1.get_counts().max() > 0
        for a, b in zip(d1.get_state() + d1.get_maps(), d2.get_state() + d2.get_maps()):
            assert np.array_equal(a, b, equal_nan=True)
        # an associating handle refuses ids
        with pytest.raises(SlamError) as e:
            d1.step(S["ctl"], np.arange(len(steps[0]["obs"])), steps[0]["obs"])
        assert e.value.code == SLAM_ERR_ARG
        with pytest.raises(SlamError):
            d1.update(np.arange(len(steps[0]["obs"])), steps[0]["obs"])
        with pytest.raises(SlamError):
            d1.load_observations([(np.arange(len(s["obs"])), s["obs"]) for s in steps])
    with DeviceFastSLAM(sc["n"], 7, noise=NOISE) as known:
        for call in (known.get_counts, lambda: known.set_counts(np.zeros(sc["n"])),
                     known.last_assoc):
            with pytest.raises(SlamError) as e:
                call()
            assert e.value.code == SLAM_ERR_ARG
    with DeviceFastSLAM(sc["n"], 7, noise=NOISE, association="ml") as quiet:   # record off
        quiet.step(S["ctl"], None, steps[0]["obs"])
        with pytest.raises(SlamError):
            quiet.last_assoc()
        with pytest.raises(SlamError):
            quiet.set_counts(np.full(sc["n"], 8))           # above the capacity


# ------------------------------------------------------------ 5. frontend
def test_frontend_builds_a_map_from_scans_without_ids():
    """FastSLAM(association="ml") on ScanSensor.scan output: every landmark of
    the best map lies near a true one.  The distance is the oracle's own: the
    float64 restatement's free run on the same scans (its own noise stream, as
    the device draws its own), its best map's largest distance to the nearest
    true landmark, doubled."""
    from conftest import PKG  # noqa: F401
    from fast_slam import FastSLAM
    from graph_based_slam import ScanSensor
    n, cap, nsteps = 2048, 24, 20
    lm = np.random.RandomState(3).uniform(-12, 12, (40, 2))
    np.random.seed(11)                                      # ScanSensor draws from the global stream
    sensor = ScanSensor(9.0, np.deg2rad(180.0), lm)
    ctl, poses = fr.circle_truth(nsteps)
    scans = [sensor.scan(p)[0] for p in poses]
    assert sum(len(s) for s in scans) > 20

    def nearest(mean):
        return float(np.max(np.min(np.hypot(mean[:, None, 0] - lm[None, :, 0],
                                            mean[:, None, 1] - lm[None, :, 1]), axis=1)))

    ref = da.FSDARef(n, cap, p_new=P_NEW, noise=NOISE, ess_th=n / 2.0)
    rs = np.random.RandomState(7)
    for sc_ in scans:
        obs = np.array([[o.getDist(), o.getDir(), o.getOrient()] for o in sc_]).reshape(-1, 3)
        out = ref.step(ctl, obs, rs.multivariate_normal([0.0, 0.0, 0.0], Q, n), rs.rand() / n)
    i = out["max_idx"]
    bound = 2.0 * nearest(ref.mean[i, :ref.cnt[i]])
    with FastSLAM(n, cap, association="ml", p_new=P_NEW, q=Q, noise=NOISE, ess_threshold=n / 2.0,
                  seed=1) as slam:
        for sc_ in scans:
            est, cov, (seen, mean, mcov) = slam.step(ctl, sc_)
        seen, mean, mcov = slam.best_map()
        assert slam.step(ctl, (None, np.zeros((0, 3))))[0].shape == (3,)
    held = seen.astype(bool)
    print(f"oracle's best map: {ref.cnt[i]} landmarks, bound {bound:.3g} m; "
          f"device's best map: {held.sum()} landmarks, worst {nearest(mean[held]):.3g} m")
    assert held.sum() >= 1 and np.array_equal(held, np.arange(cap) < held.sum())
    assert np.isfinite(mean[held]).all() and np.isnan(mean[~held]).all()
    assert nearest(mean[held]) <= bound
