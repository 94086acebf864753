"""FastSLAM on the device (slam_fs_*, slamhip.fastslam) against its NumPy
restatement, tests/fastslam_ref.py.

Bars.  Lockstep: 1e-11 relative (the C2 lockstep bar), widened to 64 x the
oracle's own float64-against-longdouble spread on the same inputs where that
is larger (the test computes the spread per scenario and quantity; the bar is
never below 1e-11).  Weights are judged relatively on entries >= 1e-280, means
absolutely against 1 + |mean|, covariances against the landmark's largest
entry, the estimate's covariance against its largest entry.  Free run:
identical decisions and argmax, x_est and the best map to 1e-9 (smoke()'s
bar), after the oracle alone has shown that no decision is within rounding.
The resampling stage is bit-exact.
"""
import numpy as np
import pytest

from conftest import ORACLE, heavy_weights  # noqa: F401

import fastslam_ref as fr
import pf_oracle as po

pytestmark = pytest.mark.gpu

NOISE = (0.1, np.deg2rad(3.0), np.deg2rad(3.0))
Q = np.diag([0.03, 0.03, np.deg2rad(2.0)]) ** 2
LD = np.longdouble

SCENARIOS = {
    # name: NP, NL, sensor range, motion, steps, empty step
    "a": dict(n=1000, nl=7, rng=9.0, motion="linear", steps=24, empty=5),
    "b": dict(n=4099, nl=12, rng=14.0, motion="velocity", steps=16, empty=None),
    "c": dict(n=513, nl=300, rng=np.inf, motion="linear", steps=3, empty=None),
}


def _rel_w(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    m = np.abs(b) >= 1e-280
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m]))) if m.any() else 0.0


def _err_mean(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b) / (1 + np.abs(b)))) if a.size else 0.0


def _err_cov(a, b):
    """[..., 3] rows against each row's largest entry."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    if not a.size:
        return 0.0
    return float(np.max(np.abs(a - b) / np.max(np.abs(b), axis=-1, keepdims=True)))


def _err_big(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _snapshot(f):
    return dict(x=f.x.copy(), y=f.y.copy(), th=f.th.copy(), w=f.w.copy(), seen=f.seen.copy(),
                mean=f.mean.copy(), cov=f.cov.copy())


def _build(name):
    """The oracle's trajectory of a scenario, computed once: per step the
    input state, the injected inputs, the float64 outputs, and the spread of
    float64 against longdouble from the same input state; beside it a free
    longdouble chain's decisions."""
    sc = SCENARIOS[name]
    n, nl = sc["n"], sc["nl"]
    lm = np.random.RandomState(3).uniform(-12, 12, (nl, 2))
    ctl, poses = fr.circle_truth(sc["steps"])
    # the stream of the injected noise: one under which the free run's oracle
    # checks hold (a resample landing on the empty step would leave every
    # weight tied at 1/NP)
    rs = np.random.RandomState(5)
    kw = dict(motion=sc["motion"], noise=NOISE, ess_th=n / 2.0)
    ref = fr.FSRef(n, nl, **kw)
    free_ld = fr.FSRef(n, nl, dtype=LD, **kw)
    spread = dict(w=0.0, mean=0.0, cov=0.0, x_est=0.0, pcov=0.0)
    steps = []
    for k, pose in enumerate(poses):
        ids, obs = fr.observe(pose, lm, sc["rng"], NOISE, rs)
        if k == sc["empty"]:
            ids, obs = ids[:0], obs[:0]
        u = rs.rand() if ref.needs_resample() else None
        ofs = None if u is None else u * (1 / n)
        noise = (rs.multivariate_normal([0.0, 0.0, 0.0], Q, n) if sc["motion"] == "linear"
                 else rs.standard_normal((n, 3)))
        pre = _snapshot(ref)
        ld = fr.FSRef(n, nl, dtype=LD, **kw)
        ld.load(ref)
        out_ld = ld.step(ctl, ids, obs, noise, ofs)
        out = ref.step(ctl, ids, obs, noise, ofs)
        assert out_ld["max_idx"] == out["max_idx"]
        spread["w"] = max(spread["w"], _rel_w(ref.w, ld.w))
        spread["mean"] = max(spread["mean"], _err_mean(ref.mean[:, ids], ld.mean[:, ids]))
        spread["cov"] = max(spread["cov"], _err_cov(ref.cov[:, ids], ld.cov[:, ids]))
        spread["x_est"] = max(spread["x_est"], _err_mean(out["x_est"], out_ld["x_est"]))
        spread["pcov"] = max(spread["pcov"], _err_big(out["cov"], out_ld["cov"]))
        ws = np.sort(ref.w)
        out_free = free_ld.step(ctl, ids, obs, noise, ofs) if free_ld.needs_resample() == \
            (u is not None) else None
        steps.append(dict(pre=pre, ids=ids, obs=obs, u=u, noise=noise, out=out,
                          post=_snapshot(ref), top_gap=float((ws[-1] - ws[-2]) / ws[-1]),
                          free_ld=None if out_free is None else
                          (out_free["resampled"], out_free["max_idx"])))
    return dict(sc=sc, ctl=ctl, steps=steps, spread=spread, final=ref, kw=kw)


_CACHE = {}


def scenario(name):
    if name not in _CACHE:
        _CACHE[name] = _build(name)
    return _CACHE[name]


def _device(sc, **kw):
    from slamhip.fastslam import DeviceFastSLAM
    return DeviceFastSLAM(sc["n"], sc["nl"], motion=sc["motion"], noise=NOISE, q=Q,
                          ess_threshold=sc["n"] / 2.0, **kw)


def _load(dev, pre):
    dev.set_state(pre["x"], pre["y"], pre["th"], pre["w"])
    dev.set_maps(pre["seen"], np.nan_to_num(pre["mean"]), np.nan_to_num(pre["cov"]))


# ---------------------------------------------------------------- 1. lockstep
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_lockstep_against_the_oracle(name):
    S = scenario(name)
    sc, steps = S["sc"], S["steps"]
    bar = {k: max(1e-11, 64 * v) for k, v in S["spread"].items()}
    print(f"scenario {name}: float64-vs-longdouble spread {S['spread']}")
    print(f"  k per step {[len(s['ids']) for s in steps]}, "
          f"resamples {sum(s['out']['resampled'] for s in steps)}")
    if name == "a":
        assert len(steps[5]["ids"]) == 0
        assert sum(s["out"]["resampled"] for s in steps) >= 2
        first = [min(k for k, s in enumerate(steps) if j in s["ids"])
                 for j in range(sc["nl"]) if any(j in s["ids"] for s in steps)]
        assert max(first) > 0, "a landmark must be first seen after step 0"
    if name == "c":
        assert all(len(s["ids"]) == 300 for s in steps)
    worst = dict.fromkeys(bar, 0.0)
    with _device(sc) as dev:
        for k, s in enumerate(steps):
            _load(dev, s["pre"])
            dev.set_resample_next(s["out"]["resampled"])
            rd = dev.step(S["ctl"], s["ids"], s["obs"], s["noise"],
                          np.nan if s["u"] is None else s["u"])
            ro, post = s["out"], s["post"]
            assert rd["resampled"] == ro["resampled"], k
            assert rd["max_idx"] == ro["max_idx"], k
            assert rd["resample_next"] == ro["resample_next"], k
            x, y, th, w = dev.get_state()
            seen, mean, cov = dev.get_maps()
            assert np.array_equal(seen.astype(bool), post["seen"]), k
            ids = s["ids"]
            err = dict(w=_rel_w(w, post["w"]), mean=_err_mean(mean[:, ids], post["mean"][:, ids]),
                       cov=_err_cov(cov[:, ids], post["cov"][:, ids]),
                       x_est=_err_mean(rd["x_est"], ro["x_est"]),
                       pcov=_err_big(rd["cov"], ro["cov"]))
            for q, e in err.items():
                worst[q] = max(worst[q], e)
                assert e <= bar[q], f"step {k}: {q} error {e:.3g} > {bar[q]:.3g}"
            # landmarks seen earlier and not observed now: untouched but for the gather
            rest = np.flatnonzero(post["seen"] & ~np.isin(np.arange(sc["nl"]), ids))
            assert np.array_equal(mean[:, rest], post["mean"][:, rest]), k
            assert np.array_equal(cov[:, rest], post["cov"][:, rest]), k
            assert np.isnan(mean[:, ~post["seen"]]).all()
    print(f"  worst device-vs-oracle errors {worst}, bars {bar}")


# ---------------------------------------------------------------- 2. free run
@pytest.mark.parametrize("name", ["a", "b"])
def test_free_run_matches_the_oracle(name):
    S = scenario(name)
    sc, steps = S["sc"], S["steps"]
    # from the oracle alone: no decision within rounding
    th = sc["n"] / 2.0
    ess_gap = min(abs(s["out"]["ess"] - th) / th for s in steps)
    top_gap = min(s["top_gap"] for s in steps)
    print(f"scenario {name}: min |ESS - ESS_TH| / ESS_TH {ess_gap:.3g}, min top-two gap {top_gap:.3g}")
    assert ess_gap > 1e-6
    assert top_gap > 1e-9
    for k, s in enumerate(steps):                      # float64 and longdouble chains agree
        assert s["free_ld"] == (s["out"]["resampled"], s["out"]["max_idx"]), k
    with _device(sc) as dev:
        for k, s in enumerate(steps):
            rd = dev.step(S["ctl"], s["ids"], s["obs"], s["noise"],
                          np.nan if s["u"] is None else s["u"])
            assert rd["resampled"] == s["out"]["resampled"], k
            assert rd["max_idx"] == s["out"]["max_idx"], k
            assert np.allclose(rd["x_est"], s["out"]["x_est"], rtol=1e-9, atol=0), k
        seen, mean, cov = dev.best_map()
        ref = S["final"]
        i = steps[-1]["out"]["max_idx"]
        assert np.array_equal(seen.astype(bool), ref.seen)
        sj = np.flatnonzero(ref.seen)
        assert _err_mean(mean[sj], ref.mean[i, sj]) <= 1e-9
        assert _err_cov(cov[sj], ref.cov[i, sj]) <= 1e-9
        assert np.isnan(mean[~ref.seen]).all() and np.isnan(cov[~ref.seen]).all()


# ------------------------------------------------- 3. resample stage, bit-exact
@pytest.mark.parametrize("n", [1, 255, 4097, 65539])
def test_resample_stage_is_bit_exact(n):
    from slamhip.fastslam import DeviceFastSLAM
    nl, u = 33, 0.37
    rs = np.random.RandomState(n)
    w = heavy_weights(rs, n)
    w = w / np.sum(w.reshape(1, n))
    x, y, th = rs.uniform(-10, 10, n), rs.uniform(-10, 10, n), rs.uniform(-3, 3, n)
    seen = np.zeros(nl, dtype=np.int32)
    seen[rs.permutation(nl)[:20]] = 1
    mean, cov = rs.uniform(-12, 12, (n, nl, 2)), rs.uniform(0.01, 2.0, (n, nl, 3))
    idx = po.systematic_indices(w, u * (1 / n))
    assert (idx >= 0).all()
    with DeviceFastSLAM(n, nl, noise=NOISE) as dev:
        dev.set_state(x, y, th, w)
        dev.set_maps(seen, mean, cov)
        assert dev.resample(u, force=True)
        gx, gy, gth, gw = dev.get_state()
        gseen, gmean, gcov = dev.get_maps()
    assert np.array_equal(gx, x[idx]) and np.array_equal(gy, y[idx]) and np.array_equal(gth, th[idx])
    assert np.array_equal(gw, np.full(n, 1 / n))
    assert np.array_equal(gseen, seen)
    sj = np.flatnonzero(seen)
    assert np.array_equal(gmean[:, sj], mean[idx][:, sj])
    assert np.array_equal(gcov[:, sj], cov[idx][:, sj])
    assert np.isnan(gmean[:, seen == 0]).all() and np.isnan(gcov[:, seen == 0]).all()


# ------------------------------------------------------------ 4. device RNG
KEYS = ("x_est", "cov", "max_val", "max_idx", "ess", "weight_sum", "resampled", "resample_next",
        "status")


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in KEYS)


def test_device_rng_is_reproducible_and_is_the_particle_filters():
    from slamhip.pf import DeviceParticleFilter
    S = scenario("a")
    sc, steps = S["sc"], S["steps"][:8]
    with _device(sc, seed=5) as d1, _device(sc, seed=5) as d2:
        for k, s in enumerate(steps):
            r1 = d1.step(S["ctl"], s["ids"], s["obs"])
            r2 = d2.step(S["ctl"], s["ids"], s["obs"])
            assert _same(r1, r2), k
        for a, b in zip(d1.get_state() + d1.get_maps(), d2.get_state() + d2.get_maps()):
            assert np.array_equal(a, b, equal_nan=True)
    lm = np.array([[5.0, 5.0], [2.0, -3.0]])
    for motion in ("linear", "velocity"):
        sc2 = dict(sc, motion=motion)
        with _device(sc2, seed=9) as d, \
                DeviceParticleFilter(sc["n"], lm, motion=motion, q=Q, seed=9,
                                     ess_threshold=sc["n"] / 2.0) as p:
            d.step(S["ctl"], steps[0]["ids"], steps[0]["obs"])
            p.step(S["ctl"], np.zeros((2, 2)))
            for a, b in zip(d.get_state()[:3], p.get_state()[:3]):
                assert np.array_equal(a, b), motion


# ---------------------------------------------------------- 5. equivalences
def test_run_equals_steps_and_stages_equal_step():
    S = scenario("a")
    sc, steps = S["sc"], S["steps"][:8]
    ctl = np.tile(S["ctl"], (len(steps), 1))
    with _device(sc, seed=3) as d1, _device(sc, seed=3) as d2:
        d1.load_observations([(s["ids"], s["obs"]) for s in steps])
        run = d1.run(0, ctl[:5]) + d1.run(5, ctl[5:])
        one = [d2.step(S["ctl"], s["ids"], s["obs"]) for s in steps]
        assert any(r["resampled"] for r in one)
        for k, (a, b) in enumerate(zip(run, one)):
            assert _same(a, b), k
        for a, b in zip(d1.get_state() + d1.get_maps(), d2.get_state() + d2.get_maps()):
            assert np.array_equal(a, b, equal_nan=True)
        t = d1.timing()
        assert set(t) == {"map_gather", "predict", "map_update", "step_end"}
        assert t["predict"] > 0 and t["step_end"] > 0
    with _device(sc, seed=4) as d1, _device(sc, seed=4) as d2:
        for k, s in enumerate(steps[:3]):
            if d1.resample_next:
                break
            d1.predict(S["ctl"])
            a = d1.update(s["ids"], s["obs"])
            b = d2.step(S["ctl"], s["ids"], s["obs"])
            assert not b["resampled"] and _same(a, b), k
            for p, q in zip(d1.get_state() + d1.get_maps(), d2.get_state() + d2.get_maps()):
                assert np.array_equal(p, q, equal_nan=True)
        assert k >= 1, "at least one non-resampling step was compared"


def test_map_accessors_agree():
    from slamhip.fastslam import DeviceFastSLAM
    n, nl = 300, 9
    rs = np.random.RandomState(2)
    seen = (rs.rand(nl) < 0.6).astype(np.int32)
    seen[0], seen[1] = 1, 0
    mean, cov = rs.uniform(-12, 12, (n, nl, 2)), rs.uniform(0.01, 2.0, (n, nl, 3))
    with DeviceFastSLAM(n, nl, noise=NOISE) as dev:
        assert dev.info() == dict(n_particles=n, n_landmarks=nl, n_seen=0)
        dev.set_maps(seen, mean, cov)
        assert dev.info()["n_seen"] == int(seen.sum())
        gseen, gmean, gcov = dev.get_maps()
        sj = seen == 1
        assert np.array_equal(gseen, seen)
        assert np.array_equal(gmean[:, sj], mean[:, sj]) and np.array_equal(gcov[:, sj], cov[:, sj])
        assert np.isnan(gmean[:, ~sj]).all() and np.isnan(gcov[:, ~sj]).all()
        for i in (0, 137, n - 1):
            s1, m1, c1 = dev.get_map(i)
            assert np.array_equal(s1, seen)
            assert np.array_equal(m1, gmean[i], equal_nan=True)
            assert np.array_equal(c1, gcov[i], equal_nan=True)
        with pytest.raises(Exception):
            dev.get_map(n)
