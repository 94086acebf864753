"""FastSLAM 2.0 on the device (slam_fs_create_proposal, fs_proposal_kernel)
against its NumPy restatement, tests/fastslam2_ref.py.

Bars are test_gpu_fastslam.py's.  Lockstep: 1e-11, widened to 64 x the oracle's
own float64-against-longdouble spread on the same inputs where that is larger
(the test computes the spread per scenario and quantity; the bar is never below
1e-11).  The proposal's mean is judged absolutely against 1 + |mu|, its
covariance against its largest entry, L absolutely against 1 + |L|; poses,
weights, maps, x_est and the particle covariance as in test_gpu_fastslam.py,
ESS relatively.  Free run: every decision of the oracle, final poses and the
best map to 1e-9, after the oracle alone has shown that no decision is within
rounding.

max_idx.  The copies of a resampled particle share mu, Sigma and L, so in a
step that resampled they carry bit-equal weights.  With T the oracle's weights
within 1e-9 relative of its maximum: |T| = 1 and the indices agree, or the
device's index lies in T and x_est is the oracle's pose at the device's index.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import ORACLE, heavy_weights  # noqa: F401

import fastslam2_ref as f2
import fastslam_ref as fr
import pf_oracle as po

pytestmark = pytest.mark.gpu

NOISE = (0.1, np.deg2rad(3.0), np.deg2rad(3.0))
Q = np.diag([0.2, 0.2, np.deg2rad(5.0)]) ** 2
LD = np.longdouble
QUANT = ("mu", "sigma", "L", "pose", "w", "mean", "cov", "x_est", "pcov", "ess")

SCENARIOS = {
    # name: NP, NL, sensor range, steps, empty step, orientation term, noise stream
    "a": dict(n=1000, nl=12, rng=9.0, steps=24, empty=5, use_orient=True, stream=5),
    "b": dict(n=4099, nl=12, rng=14.0, steps=12, empty=None, use_orient=False, stream=5),
    "c": dict(n=513, nl=300, rng=np.inf, steps=3, empty=None, use_orient=True, stream=5),
}


def _q_device():
    """Q as the handle forms it from the factor the front end hands over."""
    from slamhip.pf import numpy_noise_factor
    return f2.q_from_factor(numpy_noise_factor(Q))


def _rel_w(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    m = np.abs(b) >= 1e-280
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m]))) if m.any() else 0.0


def _err_mean(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b) / (1 + np.abs(b)))) if a.size else 0.0


def _err_cov(a, b):
    """[..., m] rows against each row's largest entry."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    if not a.size:
        return 0.0
    return float(np.max(np.abs(a - b) / np.max(np.abs(b), axis=-1, keepdims=True)))


def _err_big(a, b):
    """Against b's largest entry; absolutely where b is all zero (a single
    particle's covariance)."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    big = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (big if big > 0 else 1))


def _snapshot(f):
    return dict(x=f.x.copy(), y=f.y.copy(), th=f.th.copy(), w=f.w.copy(), seen=f.seen.copy(),
                mean=f.mean.copy(), cov=f.cov.copy())


def _record(f, out, ids):
    """What one step left behind, in the oracle's dtype."""
    return dict(mu=out["mu"], sigma=out["sigma"], L=out["L"],
                pose=np.column_stack([f.x, f.y, f.th]), w=f.w.copy(), mean=f.mean[:, ids].copy(),
                cov=f.cov[:, ids].copy(), x_est=out["x_est"], pcov=out["cov"], ess=out["ess"],
                max_idx=out["max_idx"], resampled=out["resampled"],
                resample_next=out["resample_next"])


def _ties(rec):
    """T: the oracle's weights within 1e-9 relative of its maximum."""
    w = np.asarray(rec["w"], dtype=np.float64)
    return np.flatnonzero(w >= w.max() * (1 - 1e-9))


def _errors(a, b):
    """Errors of record a against record b, per quantity; x_est against b's
    pose at a's index (b's own x_est when the indices agree)."""
    xe = np.asarray(b["pose"][a["max_idx"]], dtype=np.float64)
    return dict(mu=_err_mean(a["mu"], b["mu"]), sigma=_err_cov(a["sigma"], b["sigma"]),
                L=_err_mean(a["L"], b["L"]), pose=_err_mean(a["pose"], b["pose"]),
                w=_rel_w(a["w"], b["w"]), mean=_err_mean(a["mean"], b["mean"]),
                cov=_err_cov(a["cov"], b["cov"]), x_est=_err_mean(a["x_est"], xe),
                pcov=_err_big(a["pcov"], b["pcov"]),
                ess=abs(float(a["ess"]) - float(b["ess"])) / abs(float(b["ess"])))


def _oracle_step(pre, kw, n, nl, ctl, ids, obs, xi, ofs):
    """One step of the float64 oracle and of the longdouble one from the same
    input state: the float64 record, the state after it, and the spread."""
    ref = f2.FS2Ref(n, nl, _q_device(), **kw)
    ref.load(pre)
    ld = f2.FS2Ref(n, nl, _q_device(), dtype=LD, **kw)
    ld.load(pre)
    rec = _record(ref, ref.step(ctl, ids, obs, xi, ofs), ids)
    rec_ld = _record(ld, ld.step(ctl, ids, obs, xi, ofs), ids)
    assert rec_ld["max_idx"] in _ties(rec)
    return rec, ref, _errors(rec, rec_ld)


class _State:
    """A bare state for FSRef.load."""

    def __init__(self, d):
        self.__dict__.update(d)


def _build(name):
    """The oracle's trajectory of a scenario, computed once: per step the
    input state, the injected inputs, the float64 record and the spread of
    float64 against longdouble from the same input state; beside it a free
    longdouble chain's decisions."""
    sc = SCENARIOS[name]
    n, nl = sc["n"], sc["nl"]
    lm = np.random.RandomState(3).uniform(-12, 12, (nl, 2))
    ctl, poses = fr.circle_truth(sc["steps"])
    rs = np.random.RandomState(sc["stream"])
    kw = dict(noise=NOISE, ess_th=n / 2.0, use_orient=sc["use_orient"])
    ref = f2.FS2Ref(n, nl, _q_device(), **kw)
    free_ld = f2.FS2Ref(n, nl, _q_device(), dtype=LD, **kw)
    spread = dict.fromkeys(QUANT, 0.0)
    pivots = [np.inf] * 3
    steps = []
    for k, pose in enumerate(poses):
        ids, obs = fr.observe(pose, lm, sc["rng"], NOISE, rs)
        if k == sc["empty"]:
            ids, obs = ids[:0], obs[:0]
        u = rs.rand() if ref.needs_resample() else None
        ofs = None if u is None else u * (1 / n)
        xi = rs.standard_normal((n, 3))
        pre = _snapshot(ref)
        rec, _, sp = _oracle_step(_State(pre), kw, n, nl, ctl, ids, obs, xi, ofs)
        for q in QUANT:
            spread[q] = max(spread[q], sp[q])
        out = ref.step(ctl, ids, obs, xi, ofs)
        pivots = [min(a, b) for a, b in zip(pivots, out["pivots"])]
        agree = free_ld.needs_resample() == (u is not None)
        out_free = free_ld.step(ctl, ids, obs, xi, ofs) if agree else None
        steps.append(dict(pre=pre, ids=ids, obs=obs, u=u, xi=xi, rec=rec, post=_snapshot(ref),
                          free_ld=None if out_free is None else out_free["resampled"]))
    return dict(sc=sc, ctl=ctl, steps=steps, spread=spread, final=ref, kw=kw, pivots=pivots)


_CACHE = {}


def scenario(name):
    if name not in _CACHE:
        _CACHE[name] = _build(name)
    return _CACHE[name]


def _device(n, nl, **kw):
    from slamhip.fastslam import DeviceFastSLAM
    kw.setdefault("ess_threshold", n / 2.0)
    return DeviceFastSLAM(n, nl, noise=NOISE, q=Q, proposal="measurement", **kw)


def _load(dev, pre):
    dev.set_state(pre["x"], pre["y"], pre["th"], pre["w"])
    dev.set_maps(pre["seen"], np.nan_to_num(pre["mean"]), np.nan_to_num(pre["cov"]))


def _device_record(dev, rd, ids):
    mu, sigma, L = dev.last_proposal()
    x, y, th, w = dev.get_state()
    seen, mean, cov = dev.get_maps()
    rec = dict(mu=mu, sigma=sigma, L=L, pose=np.column_stack([x, y, th]), w=w, mean=mean[:, ids],
               cov=cov[:, ids], x_est=rd["x_est"], pcov=rd["cov"], ess=rd["ess"],
               max_idx=rd["max_idx"], resampled=rd["resampled"], resample_next=rd["resample_next"])
    return rec, seen, mean, cov


def _check_step(dev, rd, rec, post, ids, nl, bar, worst, tag):
    """One device step against the oracle's record of the same inputs."""
    drec, seen, mean, cov = _device_record(dev, rd, ids)
    assert drec["resampled"] == rec["resampled"], tag
    assert drec["resample_next"] == rec["resample_next"], tag
    T = _ties(rec)
    if T.size == 1:
        assert drec["max_idx"] == rec["max_idx"], tag
    else:
        assert drec["max_idx"] in T, tag
    assert np.array_equal(seen.astype(bool), post["seen"]), tag
    for q, e in _errors(drec, rec).items():
        worst[q] = max(worst[q], e)
        assert e <= bar[q], f"{tag}: {q} error {e:.3g} > {bar[q]:.3g}"
    # landmarks seen earlier and not observed now: untouched but for the gather
    rest = np.flatnonzero(post["seen"] & ~np.isin(np.arange(nl), ids))
    assert np.array_equal(mean[:, rest], post["mean"][:, rest]), tag
    assert np.array_equal(cov[:, rest], post["cov"][:, rest]), tag
    assert np.isnan(mean[:, ~post["seen"]]).all(), tag


# ---------------------------------------------------------------- 1. lockstep
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_lockstep_against_the_oracle(name):
    S = scenario(name)
    sc, steps = S["sc"], S["steps"]
    bar = {k: max(1e-11, 64 * v) for k, v in S["spread"].items()}
    print(f"scenario {name}: float64-vs-longdouble spread {S['spread']}")
    print(f"  k per step {[len(s['ids']) for s in steps]}, "
          f"resamples {sum(s['rec']['resampled'] for s in steps)}, smallest pivots {S['pivots']}")
    if name == "a":
        assert len(steps[5]["ids"]) == 0
        assert sum(s["rec"]["resampled"] for s in steps) >= 2
        first = [min(k for k, s in enumerate(steps) if j in s["ids"])
                 for j in range(sc["nl"]) if any(j in s["ids"] for s in steps)]
        assert max(first) > 0, "a landmark must be first seen after step 0"
    if name == "c":
        assert all(len(s["ids"]) == 300 for s in steps)
    worst = dict.fromkeys(bar, 0.0)
    with _device(sc["n"], sc["nl"], use_orient=sc["use_orient"], record_proposal=True) as dev:
        for k, s in enumerate(steps):
            _load(dev, s["pre"])
            dev.set_resample_next(s["rec"]["resampled"])
            rd = dev.step(S["ctl"], s["ids"], s["obs"], s["xi"],
                          np.nan if s["u"] is None else s["u"])
            _check_step(dev, rd, s["rec"], s["post"], s["ids"], sc["nl"], bar, worst, f"step {k}")
    print(f"  worst device-vs-oracle errors {worst}, bars {bar}")


# ---------------------------------------------------------------- 2. free run
@pytest.mark.parametrize("name", ["a", "b"])
def test_free_run_matches_the_oracle(name):
    S = scenario(name)
    sc, steps = S["sc"], S["steps"]
    n = sc["n"]
    # from the oracle alone: no resample decision within rounding
    ess_gap = min(abs(s["rec"]["ess"] - n / 2.0) for s in steps) / n
    print(f"scenario {name}: min |ESS - ESS_TH| / NP {ess_gap:.3g}")
    assert ess_gap >= 1e-6
    for k, s in enumerate(steps):                      # float64 and longdouble chains decide alike
        assert s["free_ld"] == s["rec"]["resampled"], k
    assert any(s["rec"]["resampled"] for s in steps)
    with _device(n, sc["nl"], use_orient=sc["use_orient"]) as dev:
        for k, s in enumerate(steps):
            rd = dev.step(S["ctl"], s["ids"], s["obs"], s["xi"],
                          np.nan if s["u"] is None else s["u"])
            assert rd["resampled"] == s["rec"]["resampled"], k
            assert rd["resample_next"] == s["rec"]["resample_next"], k
        ref, last = S["final"], steps[-1]["rec"]
        i = rd["max_idx"]
        assert i in _ties(last)
        x, y, th, _ = dev.get_state()
        assert _err_mean(np.column_stack([x, y, th]), last["pose"]) <= 1e-9
        assert _err_mean(rd["x_est"], last["pose"][i]) <= 1e-9
        seen, mean, cov = dev.best_map()
        assert np.array_equal(seen.astype(bool), ref.seen)
        sj = np.flatnonzero(ref.seen)
        assert _err_mean(mean[sj], ref.mean[i, sj]) <= 1e-9
        assert _err_cov(cov[sj], ref.cov[i, sj]) <= 1e-9
        assert np.isnan(mean[~ref.seen]).all() and np.isnan(cov[~ref.seen]).all()


# ------------------------------------------------------------------- 3. edges
def _set_state(n, nl, seed):
    """Scattered poses, near-uniform weights, and a map of the even landmarks."""
    rs = np.random.RandomState(seed)
    lm = rs.uniform(-12, 12, (nl, 2))
    seen = (np.arange(nl) % 2 == 0)
    mean = np.full((n, nl, 2), np.nan)
    cov = np.full((n, nl, 3), np.nan)
    mean[:, seen] = lm[seen] + rs.normal(0, 0.1, (n, int(seen.sum()), 2))
    a = rs.normal(0, 0.1, (n, int(seen.sum()), 2, 2))
    P = a @ np.swapaxes(a, -1, -2) + 0.01 * np.eye(2)
    cov[:, seen] = np.stack([P[..., 0, 0], P[..., 0, 1], P[..., 1, 1]], axis=-1)
    w = rs.uniform(0.5, 1.5, n)
    pre = dict(x=10.0 + rs.normal(0, 0.2, n), y=rs.normal(0, 0.2, n),
               th=np.pi / 2 + rs.normal(0, 0.05, n), w=w / np.sum(w.reshape(1, n)), seen=seen,
               mean=mean, cov=cov)
    return lm, pre, rs


def test_block_and_observation_count_edges():
    """NP across the block edge and k across the LDS pass (128), one step each
    from a set state with seen and unseen landmarks in the scan."""
    nl = 130
    ctl = fr.circle_truth(1)[0]
    truth = np.array([10.0, 0.17, np.pi / 2 + 0.017])
    for n in (1, 2, 255, 257):
        lm, pre, rs = _set_state(n, nl, 100 + n)
        ids_all, obs_all = fr.observe(truth, lm, np.inf, NOISE, rs)
        xi = rs.standard_normal((n, 3))
        kw = dict(noise=NOISE, ess_th=n / 100.0, use_orient=True)
        with _device(n, nl, ess_threshold=n / 100.0, record_proposal=True) as dev:
            for k in (0, 1, 128, 129):
                ids, obs = ids_all[:k], obs_all[:k]
                assert k < 2 or (pre["seen"][ids].any() and not pre["seen"][ids].all())
                rec, ref, sp = _oracle_step(_State(pre), kw, n, nl, ctl, ids, obs, xi, None)
                assert not rec["resampled"]
                bar = {q: max(1e-11, 64 * v) for q, v in sp.items()}
                _load(dev, pre)
                dev.set_resample_next(False)
                rd = dev.step(ctl, ids, obs, xi)
                worst = dict.fromkeys(bar, 0.0)
                _check_step(dev, rd, rec, _snapshot(ref), ids, nl, bar, worst, f"NP {n}, k {k}")
                print(f"NP {n}, k {k}: worst {worst}")


# -------------------------------------------------------------- 4. device RNG
def _normals(n, rstep, seed):
    from slamhip import _lib
    pairs = (n + 1) // 2
    out = np.empty((pairs, 6))
    _lib.check(_lib.load().slam_debug_pair_normals(0, 0, pairs, rstep, seed,
                                                   out.ctypes.data_as(C.POINTER(C.c_double))),
               "slam_debug_pair_normals")
    return out.reshape(2 * pairs, 3)[:n]


def test_device_rng_draws_the_predicts_normals():
    """noise = None: particle 2p takes the first three, 2p + 1 the last three
    of pair_normals(p, step number, seed); NP odd, so the last pair is half
    used.  The oracle is re-based on the device's state before every step and
    fed the same normals."""
    n, nl, seed = 4099, 12, 7
    lm = np.random.RandomState(3).uniform(-12, 12, (nl, 2))
    ctl, poses = fr.circle_truth(4)
    rs = np.random.RandomState(9)
    kw = dict(noise=NOISE, ess_th=n / 100.0, use_orient=True)
    with _device(n, nl, ess_threshold=n / 100.0, seed=seed, record_proposal=True) as dev:
        for k, pose in enumerate(poses):
            ids, obs = fr.observe(pose, lm, 9.0, NOISE, rs)
            x, y, th, w = dev.get_state()
            seen, mean, cov = dev.get_maps()
            pre = dict(x=x, y=y, th=th, w=w, seen=seen.astype(bool), mean=mean, cov=cov)
            xi = _normals(n, k, seed)
            rec, ref, sp = _oracle_step(_State(pre), kw, n, nl, ctl, ids, obs, xi, None)
            assert not rec["resampled"]
            bar = {q: max(1e-11, 64 * v) for q, v in sp.items()}
            rd = dev.step(ctl, ids, obs)
            _check_step(dev, rd, rec, _snapshot(ref), ids, nl, bar, dict.fromkeys(bar, 0.0),
                        f"step {k}")


# ---------------------------------------------------------- 5. equivalences
KEYS = ("x_est", "cov", "max_val", "max_idx", "ess", "weight_sum", "resampled", "resample_next",
        "status")


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in KEYS)


def test_run_equals_steps():
    S = scenario("a")
    steps = S["steps"][:6]
    n, nl = S["sc"]["n"], S["sc"]["nl"]
    ctl = np.tile(S["ctl"], (len(steps), 1))
    with _device(n, nl, seed=3) as d1, _device(n, nl, seed=3) as d2:
        d1.load_observations([(s["ids"], s["obs"]) for s in steps])
        run = d1.run(0, ctl[:4]) + d1.run(4, ctl[4:])
        one = [d2.step(S["ctl"], s["ids"], s["obs"]) for s in steps]
        for k, (a, b) in enumerate(zip(run, one)):
            assert _same(a, b), k
        for a, b in zip(d1.get_state() + d1.get_maps(), d2.get_state() + d2.get_maps()):
            assert a.tobytes() == b.tobytes()
        t = d1.timing()
        assert set(t) == {"map_gather", "predict", "map_update", "step_end"}
        assert t["predict"] > 0 and t["step_end"] > 0
        assert d1.info()["n_seen"] == d2.info()["n_seen"] > 0


@pytest.mark.parametrize("n", [255, 4097])
def test_resample_stage_is_bit_exact(n):
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
    with _device(n, nl) as dev:
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


def test_stage_calls_and_accessors_refuse_the_wrong_handle():
    from slamhip._lib import SlamError
    from slamhip.fastslam import DeviceFastSLAM
    S = scenario("a")
    s = S["steps"][0]
    with _device(100, 12) as new, _device(100, 12, record_proposal=True) as rec, \
            DeviceFastSLAM(100, 12, noise=NOISE, q=Q) as old:
        with pytest.raises(SlamError):
            new.predict(S["ctl"])
        with pytest.raises(SlamError):
            new.update(s["ids"], s["obs"])
        with pytest.raises(SlamError):
            old.last_proposal()
        with pytest.raises(SlamError):
            new.last_proposal()                        # created without record
        with pytest.raises(SlamError):
            rec.last_proposal()                        # no step yet
        for h in (new, old):
            with pytest.raises(SlamError):
                h.get_counts()
            with pytest.raises(SlamError):
                h.last_assoc()
        rec.step(S["ctl"], s["ids"], s["obs"])
        mu, sigma, L = rec.last_proposal()
        assert np.isfinite(mu).all() and np.isfinite(sigma).all() and np.isfinite(L).all()


def test_frontend_steps_the_docstring_world():
    from conftest import PKG  # noqa: F401
    from fast_slam import FastSLAM
    from graph_based_slam import ScanSensor
    lm = np.random.RandomState(3).uniform(-12, 12, (7, 2))
    sensor = ScanSensor(9.0, np.deg2rad(180.0), lm)
    v, w, dt = 10.0 * np.deg2rad(10.0), np.deg2rad(10.0), 0.1
    pose = np.array([10.0, 0.0, np.pi / 2])
    np.random.seed(4)
    observed = np.zeros(len(lm), dtype=int)
    with FastSLAM(4096, len(lm), ess_threshold=2048, seed=1, proposal="measurement") as slam:
        for _ in range(30):
            pose = pose + np.array([v * dt * np.cos(pose[2]), v * dt * np.sin(pose[2]), w * dt])
            noisy, _ = sensor.scan(pose)
            observed[[o.getLandMarkId() for o in noisy]] += 1
            est, cov, (seen, mean, mcov) = slam.step((v, w), noisy)
        seen, mean, mcov = slam.best_map()
        assert int(seen.sum()) == int((observed > 0).sum()) > 0
        assert np.array_equal(seen.astype(bool), observed > 0)
        assert np.isfinite(mean[observed > 0]).all() and np.isnan(mean[observed == 0]).all()
        assert np.isfinite(est).all() and np.hypot(*(est[:2] - pose[:2])) < 1.0
