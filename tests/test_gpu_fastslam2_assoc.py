"""FastSLAM 2.0 without ids on the device (slam_fs_create_assoc_proposal,
fs_assoc_proposal_kernel, slamhip.fastslam association="ml_marginal") against
its NumPy restatement, tests/fastslam2_da_ref.py.

Bars.  Precondition, on the oracle alone and before the device is touched:
from every step's input state float64 and longdouble make identical choices
and counts, and the smallest finite decision margin is at least 1e-8 (far above
fp64 rounding of a score) -- the device must then make every choice and count
exactly.  The margin is |l_best - log_p_new|, and l_best - l_second as well
where the best candidate is taken.  Lockstep values: test_gpu_fastslam.py's
measures and bar, 1e-11 widened to 64 x the oracle's own float64-against-
longdouble spread per scenario and quantity (the proposal's mean against
1 + |mu|, its covariance against its largest entry, L against 1 + |L|).
max_idx: the copies of a resampled particle carry bit-equal weights, so with T
the oracle's weights within 1e-9 relative of its maximum, |T| = 1 and the
indices agree, or the device's index lies in T and x_est is the oracle's pose
at the device's index.  Free run: every resample decision, choice and count of
the oracle, final poses and the best map to 1e-9, after the oracle alone has
shown that no ESS is within 1e-9 NP of the threshold.  The resampling stage
and run-against-step are bit-exact.

The oracle's own figures on these inputs (stream 5): smallest margins A 2.9e-7,
B 2.3e-5, C 2.5e-7, D 5.4e-6; resamplings A 8, B 5, C 8, D 0; min |ESS -
ESS_TH| / NP A 2.0e-2, B 2.0e-3, C 3.3e-2; 2,084,688 choices in all, 624,423 of
them dropped.  Measured on an MI355X, weights / means / covariances / mu /
Sigma / L: the oracle's spread A 5.6e-14 / 9.4e-15 / 2.3e-15 / 7.3e-16 / 1.2e-15
/ 2.8e-15, B 3.6e-14 / 1.3e-15 / 1.5e-15 / 6.4e-16 / 1.4e-15 / 6.9e-15, C 6.3e-14
/ 1.0e-14 / 2.3e-15 / 9.6e-16 / 1.3e-15 / 9.2e-15, D 2.6e-13 / 1.7e-14 / 1.3e-14 /
2.2e-15 / 3.1e-15 / 1.3e-14; the device's worst errors A 2.2e-14 / 2.1e-15 /
1.5e-15 / 4.4e-16 / 9.4e-16 / 1.1e-15, B 2.5e-14 / 7.1e-16 / 1.4e-15 / 3.5e-16 /
5.9e-16 / 3.4e-15, C 2.9e-14 / 3.0e-15 / 2.0e-15 / 3.2e-16 / 5.4e-16 / 3.1e-15, D
1.5e-14 / 5.1e-15 / 2.2e-15 / 3.7e-16 / 4.3e-16 / 4.0e-16.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ORACLE, heavy_weights  # noqa: F401

import fastslam2_da_ref as d2
import fastslam_ref as fr
import pf_oracle as po
from test_gpu_fastslam2 import (NOISE, Q, LD, _q_device, _rel_w, _err_mean, _err_cov, _err_big,
                                _ties, _normals, _same)

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
QUANT = ("mu", "sigma", "L", "pose", "w", "mean", "cov", "x_est", "pcov", "ess")


def _held(a, cnt):
    """[n][cap][c] -> the rows below each particle's count, flattened."""
    return a[np.arange(a.shape[1])[None, :] < cnt[:, None]]


def _record(f, out):
    """What one step left behind, in the oracle's dtype."""
    return dict(mu=out["mu"], sigma=out["sigma"], L=out["L"],
                pose=np.column_stack([f.x, f.y, f.th]), w=f.w.copy(), cnt=f.cnt.copy(),
                mean=f.mean.copy(), cov=f.cov.copy(), x_est=out["x_est"], pcov=out["cov"],
                ess=out["ess"], max_idx=out["max_idx"], resampled=out["resampled"],
                resample_next=out["resample_next"], assoc=out["assoc"], idx=out.get("idx"))


def _errors(a, b):
    """Errors of record a against record b (equal counts), per quantity; x_est
    against b's pose at a's index (b's own x_est when the indices agree)."""
    cnt = b["cnt"]
    xe = np.asarray(b["pose"][a["max_idx"]], dtype=np.float64)
    return dict(mu=_err_mean(a["mu"], b["mu"]), sigma=_err_cov(a["sigma"], b["sigma"]),
                L=_err_mean(a["L"], b["L"]), pose=_err_mean(a["pose"], b["pose"]),
                w=_rel_w(a["w"], b["w"]),
                mean=_err_mean(_held(a["mean"], cnt), _held(b["mean"], cnt)),
                cov=_err_cov(_held(a["cov"], cnt), _held(b["cov"], cnt)),
                x_est=_err_mean(a["x_est"], xe), pcov=_err_big(a["pcov"], b["pcov"]),
                ess=abs(float(a["ess"]) - float(b["ess"])) / abs(float(b["ess"])))


def _oracle(n, cap, kw, dtype=np.float64, pre=None):
    ref = d2.FS2DARef(n, cap, _q_device(), dtype=dtype, **kw)
    if pre is not None:
        for k in ("x", "y", "th", "w", "mean", "cov"):
            setattr(ref, k, pre[k].astype(dtype))
        ref.cnt = pre["cnt"].copy()
    return ref


def _against_longdouble(rec, pre, kw, n, cap, ctl, obs, xi, ofs):
    """The step again in longdouble from the float64 input state: whether the
    two decide alike, and the spread."""
    ld = _oracle(n, cap, kw, LD, pre)
    rec_ld = _record(ld, ld.step(ctl, obs, xi, ofs))
    same = bool(np.array_equal(rec["assoc"], rec_ld["assoc"]) and
                np.array_equal(rec["cnt"], rec_ld["cnt"]) and rec_ld["max_idx"] in _ties(rec))
    return same, _errors(rec, rec_ld) if same else {}


def _min_margin(out):
    fin = out["margin"][np.isfinite(out["margin"])]
    return float(fin.min()) if fin.size else np.inf


def _oracle_step(pre, kw, n, cap, ctl, obs, xi, ofs):
    """One step of the float64 oracle and of the longdouble one from the same
    input state: the float64 record, the smallest finite margin, whether the
    two decide alike, and the spread."""
    ref = _oracle(n, cap, kw, pre=pre)
    out = ref.step(ctl, obs, xi, ofs)
    rec = _record(ref, out)
    same, sp = _against_longdouble(rec, pre, kw, n, cap, ctl, obs, xi, ofs)
    return rec, _min_margin(out), same, sp, out["pivots"]


def _build(name):
    """The oracle's trajectory of a scenario, computed once: per step the input
    state, the injected inputs, the float64 record, whether longdouble from the
    same input state decides identically, and the float64-against-longdouble
    spread."""
    sc = SCENARIOS[name]
    n, cap = sc["n"], sc["cap"]
    lm = np.random.RandomState(3).uniform(-12, 12, (sc["nl"], 2))
    ctl, poses = fr.circle_truth(sc["steps"])
    rs = np.random.RandomState(5)
    kw = dict(p_new=P_NEW, noise=NOISE, ess_th=n / 2.0)
    ref = _oracle(n, cap, kw)
    steps, pivots = [], [np.inf] * 3
    for pose in poses:
        _, obs = fr.observe(pose, lm, sc["rng"], NOISE, rs)
        u = rs.rand()
        xi = rs.standard_normal((n, 3))
        pre = ref.snapshot()
        out = ref.step(ctl, obs, xi, u * (1 / n))
        pivots = [min(a, b) for a, b in zip(pivots, out["pivots"])]
        steps.append(dict(pre=pre, obs=obs, u=u, xi=xi, rec=_record(ref, out),
                          min_margin=_min_margin(out)))

    def against(s):
        """(the steps are independent, and NumPy's longdouble loops release the GIL)"""
        return _against_longdouble(s["rec"], s["pre"], kw, n, cap, ctl, s["obs"], s["xi"],
                                   s["u"] * (1 / n))

    spread = dict.fromkeys(QUANT, 0.0)
    with ThreadPoolExecutor(max_workers=8) as pool:
        for s, (same, sp) in zip(steps, pool.map(against, steps)):
            s["same_ld"] = same
            for q, v in sp.items():
                spread[q] = max(spread[q], v)
    return dict(sc=sc, ctl=ctl, steps=steps, spread=spread, final=ref, kw=kw, pivots=pivots)


_CACHE = {}


def scenario(name):
    if name not in _CACHE:
        _CACHE[name] = _build(name)
    return _CACHE[name]


def _precondition(name):
    """On the oracle alone: every decision is decided well above rounding."""
    S = scenario(name)
    steps = S["steps"]
    a = np.concatenate([s["rec"]["assoc"].ravel() for s in steps])
    mm = min(s["min_margin"] for s in steps)
    disagree = sum(int((s["rec"]["assoc"] != s["rec"]["assoc"][:, :1]).any(axis=1).sum())
                   for s in steps)
    th = S["sc"]["n"] / 2.0
    print(f"scenario {name}: {a.size} choices, {int((a == d2.DROPPED).sum())} dropped, "
          f"{int((a == d2.NEW).sum())} new, smallest margin {mm:.3g}, "
          f"resamplings {sum(s['rec']['resampled'] for s in steps)}, "
          f"min |ESS - ESS_TH| / NP {min(abs(s['rec']['ess'] - th) for s in steps) / S['sc']['n']:.3g}, "
          f"final counts {S['final'].cnt.min()}..{S['final'].cnt.max()}, "
          f"observations the particles disagree about {disagree}, smallest pivots {S['pivots']}")
    for k, s in enumerate(steps):
        assert s["same_ld"], f"step {k}: float64 and longdouble decide differently"
    assert mm >= MARGIN_BAR, f"smallest decision margin {mm:.3g} < {MARGIN_BAR}"
    return S


def _device(n, cap, **kw):
    from slamhip.fastslam import DeviceFastSLAM
    kw.setdefault("ess_threshold", n / 2.0)
    kw.setdefault("record_assoc", True)
    kw.setdefault("record_proposal", True)
    return DeviceFastSLAM(n, cap, noise=NOISE, q=Q, association="ml_marginal",
                          proposal="measurement", p_new=P_NEW, **kw)


def _load(dev, pre):
    dev.set_state(pre["x"], pre["y"], pre["th"], pre["w"])
    dev.set_maps(None, np.nan_to_num(pre["mean"]), np.nan_to_num(pre["cov"]))
    dev.set_counts(pre["cnt"])


def _nan_above(a, cnt):
    return bool(np.isnan(a[np.arange(a.shape[1])[None, :] >= cnt[:, None]]).all())


def _check_step(dev, rd, rec, pre, bar, worst, tag):
    """One device step against the oracle's record of the same inputs."""
    n, cap = rec["mean"].shape[:2]
    assert rd["resampled"] == rec["resampled"], tag
    if rec["assoc"].shape[0]:
        assert np.array_equal(dev.last_assoc(), rec["assoc"]), tag
    cnt = dev.get_counts()
    assert np.array_equal(cnt, rec["cnt"]), tag
    assert rd["resample_next"] == rec["resample_next"], tag
    T = _ties(rec)
    if T.size == 1:
        assert rd["max_idx"] == rec["max_idx"], tag
    else:
        assert rd["max_idx"] in T, tag
    mu, sigma, L = dev.last_proposal()
    x, y, th, w = dev.get_state()
    seen, mean, cov = dev.get_maps()
    assert np.array_equal(seen, (np.arange(cap) < cnt.max()).astype(np.int32)), tag
    assert dev.info() == dict(n_particles=n, n_landmarks=cap, n_seen=int(cnt.max())), tag
    drec = dict(mu=mu, sigma=sigma, L=L, pose=np.column_stack([x, y, th]), w=w, cnt=cnt, mean=mean,
                cov=cov, x_est=rd["x_est"], pcov=rd["cov"], ess=rd["ess"], max_idx=rd["max_idx"])
    for q, e in _errors(drec, rec).items():
        worst[q] = max(worst[q], e)
        assert e <= bar[q], f"{tag}: {q} error {e:.3g} > {bar[q]:.3g}"
    assert _nan_above(mean, cnt) and _nan_above(cov, cnt), tag
    # slots no observation matched or created: untouched but for the gather
    touched = np.zeros((n, cap), dtype=bool)
    a = rec["assoc"]
    for q in range(a.shape[0]):
        pm = np.flatnonzero(a[q] >= 0)
        touched[pm, a[q, pm]] = True
    base = pre["cnt"][rec["idx"]] if rec["resampled"] else pre["cnt"]
    rest = ~touched & (np.arange(cap)[None, :] < base[:, None])
    assert np.array_equal(mean[rest], rec["mean"][rest]), tag
    assert np.array_equal(cov[rest], rec["cov"][rest]), tag


# ---------------------------------------------------------------- 1. lockstep
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_lockstep_against_the_oracle(name):
    S = _precondition(name)
    sc, steps = S["sc"], S["steps"]
    bar = {k: max(1e-11, 64 * v) for k, v in S["spread"].items()}
    print(f"  float64-vs-longdouble spread {S['spread']}")
    print(f"  k per step {[len(s['obs']) for s in steps]}")
    if name == "B":
        assert any((s["rec"]["assoc"] == d2.DROPPED).any() for s in steps[:8]), "full early"
    if name == "D":
        assert all(len(s["obs"]) == 300 for s in steps)
        assert (steps[0]["rec"]["assoc"] == d2.DROPPED).any(), "overflow from the first step"
    worst = dict.fromkeys(bar, 0.0)
    with _device(sc["n"], sc["cap"]) as dev:
        assert dev.info() == dict(n_particles=sc["n"], n_landmarks=sc["cap"], n_seen=0)
        for k, s in enumerate(steps):
            _load(dev, s["pre"])
            dev.set_resample_next(s["rec"]["resampled"])
            rd = dev.step(S["ctl"], None, s["obs"], s["xi"], s["u"])
            _check_step(dev, rd, s["rec"], s["pre"], bar, worst, f"step {k}")
    print(f"  worst device-vs-oracle errors {worst}, bars {bar}")


# ---------------------------------------------------------------- 2. free run
@pytest.mark.parametrize("name", ["A", "C"])
def test_free_run_matches_the_oracle(name):
    S = _precondition(name)
    sc, steps = S["sc"], S["steps"]
    n = sc["n"]
    ess_gap = min(abs(s["rec"]["ess"] - n / 2.0) for s in steps) / n
    print(f"scenario {name}: min |ESS - ESS_TH| / NP {ess_gap:.3g}")
    assert ess_gap > 1e-9
    assert any(s["rec"]["resampled"] for s in steps)
    with _device(n, sc["cap"], record_proposal=False, record_assoc=False) as dev:
        for k, s in enumerate(steps):
            rd = dev.step(S["ctl"], None, s["obs"], s["xi"], s["u"])
            assert rd["resampled"] == s["rec"]["resampled"], k
            assert rd["resample_next"] == s["rec"]["resample_next"], k
            assert np.array_equal(dev.last_assoc(), s["rec"]["assoc"]), k     # record off: still kept
            assert np.array_equal(dev.get_counts(), s["rec"]["cnt"]), k
        ref, last = S["final"], steps[-1]["rec"]
        i = rd["max_idx"]
        assert i in _ties(last)
        x, y, th, _ = dev.get_state()
        assert _err_mean(np.column_stack([x, y, th]), last["pose"]) <= 1e-9
        assert _err_mean(rd["x_est"], last["pose"][i]) <= 1e-9
        seen, mean, cov = dev.best_map()
        c = int(ref.cnt[i])
        assert np.array_equal(seen, (np.arange(sc["cap"]) < c).astype(np.int32))
        assert _err_mean(mean[:c], ref.mean[i, :c]) <= 1e-9
        assert _err_cov(cov[:c], ref.cov[i, :c]) <= 1e-9
        assert np.isnan(mean[c:]).all() and np.isnan(cov[c:]).all()


# ------------------------------------------------------------------- 3. edges
def _set_state(n, cap, nl, seed):
    """Scattered poses, near-uniform weights, and per particle a map of its
    first cnt landmarks of the world (cnt varies inside a wave, 0 and cap
    included)."""
    rs = np.random.RandomState(seed)
    lm = rs.uniform(-12, 12, (nl, 2))
    cnt = rs.randint(0, cap + 1, n).astype(np.int32)
    cnt[::7] = 0
    cnt[1::7] = cap // 2
    cnt[3::7] = cap
    mean = lm[None, :cap] + rs.normal(0, 0.1, (n, cap, 2))
    a = rs.normal(0, 0.1, (n, cap, 2, 2))
    P = a @ np.swapaxes(a, -1, -2) + 0.01 * np.eye(2)
    cov = np.stack([P[..., 0, 0], P[..., 0, 1], P[..., 1, 1]], axis=-1)
    above = np.arange(cap)[None, :] >= cnt[:, None]
    mean[above], cov[above] = np.nan, np.nan
    w = rs.uniform(0.5, 1.5, n)
    pre = dict(x=10.0 + rs.normal(0, 0.2, n), y=rs.normal(0, 0.2, n),
               th=np.pi / 2 + rs.normal(0, 0.05, n), w=w / np.sum(w.reshape(1, n)), cnt=cnt,
               mean=mean, cov=cov)
    return lm, pre, rs


@pytest.mark.parametrize("n", [1, 2, 255, 257])
def test_block_and_observation_count_edges(n):
    """NP across the block edge and k across the LDS pass (128), one step each
    from a set state whose counts run from 0 to the capacity inside a wave:
    the jmax masking, the padding lanes, the pass boundary and the drop path."""
    cap, nl = 8, 130
    ctl = fr.circle_truth(1)[0]
    truth = np.array([10.0, 0.17, np.pi / 2 + 0.017])
    lm, pre, rs = _set_state(n, cap, nl, 100 + n)
    _, obs_all = fr.observe(truth, lm, np.inf, NOISE, rs)
    xi = rs.standard_normal((n, 3))
    kw = dict(p_new=P_NEW, noise=NOISE, ess_th=n / 100.0)
    cases = []
    for k in (0, 1, 128, 129):
        rec, mm, same, sp, _ = _oracle_step(pre, kw, n, cap, ctl, obs_all[:k], xi, None)
        assert same and mm >= MARGIN_BAR, (k, same, mm)
        assert not rec["resampled"]
        cases.append((k, rec, sp))
    a = cases[-1][1]["assoc"]
    if n > 2:
        assert (a >= 0).any() and (a == d2.NEW).any() and (a == d2.DROPPED).any()
    with _device(n, cap, ess_threshold=n / 100.0) as dev:
        for k, rec, sp in cases:
            bar = {q: max(1e-11, 64 * v) for q, v in sp.items()}
            _load(dev, pre)
            dev.set_resample_next(False)
            rd = dev.step(ctl, None, obs_all[:k], xi)
            worst = dict.fromkeys(bar, 0.0)
            _check_step(dev, rd, rec, pre, bar, worst, f"NP {n}, k {k}")
            print(f"NP {n}, k {k}: worst {worst}")


# -------------------------------------------------------------- 4. device RNG
def test_device_rng_draws_the_predicts_normals():
    """noise = None: particle 2p takes the first three, 2p + 1 the last three
    of pair_normals(p, step number, seed); NP odd, so the last pair is half
    used.  The oracle is re-based on the device's state before every step and
    fed the same normals."""
    n, cap, seed = 4099, 16, 7
    lm = np.random.RandomState(3).uniform(-12, 12, (40, 2))
    ctl, poses = fr.circle_truth(4)
    rs = np.random.RandomState(9)
    kw = dict(p_new=P_NEW, noise=NOISE, ess_th=n / 100.0)
    with _device(n, cap, ess_threshold=n / 100.0, seed=seed) as dev:
        for k, pose in enumerate(poses):
            _, obs = fr.observe(pose, lm, 9.0, NOISE, rs)
            x, y, th, w = dev.get_state()
            _, mean, cov = dev.get_maps()
            pre = dict(x=x, y=y, th=th, w=w, cnt=dev.get_counts(), mean=mean, cov=cov)
            xi = _normals(n, k, seed)
            rec, mm, same, sp, _ = _oracle_step(pre, kw, n, cap, ctl, obs, xi, None)
            assert same and mm >= MARGIN_BAR, (k, same, mm)
            assert not rec["resampled"]
            bar = {q: max(1e-11, 64 * v) for q, v in sp.items()}
            rd = dev.step(ctl, None, obs)
            _check_step(dev, rd, rec, pre, bar, dict.fromkeys(bar, 0.0), f"step {k}")
        assert dev.get_counts().max() > 0


# ---------------------------------------------------------- 5. equivalences
@pytest.mark.parametrize("n", [255, 4097])
def test_resample_stage_is_bit_exact(n):
    cap, u = 33, 0.37
    rs = np.random.RandomState(n)
    w = heavy_weights(rs, n)
    w = w / np.sum(w.reshape(1, n))
    x, y, th = rs.uniform(-10, 10, n), rs.uniform(-10, 10, n), rs.uniform(-3, 3, n)
    cnt = rs.randint(0, cap + 1, n).astype(np.int32)
    mean, cov = rs.uniform(-12, 12, (n, cap, 2)), rs.uniform(0.01, 2.0, (n, cap, 3))
    idx = po.systematic_indices(w, u * (1 / n))
    assert (idx >= 0).all()
    with _device(n, cap) as dev:
        dev.set_state(x, y, th, w)
        dev.set_maps(None, mean, cov)
        dev.set_counts(cnt)
        assert dev.resample(u, force=True)
        gx, gy, gth, gw = dev.get_state()
        gcnt = dev.get_counts()
        gseen, gmean, gcov = dev.get_maps()
    assert np.array_equal(gx, x[idx]) and np.array_equal(gy, y[idx]) and np.array_equal(gth, th[idx])
    assert np.array_equal(gw, np.full(n, 1 / n))
    assert np.array_equal(gcnt, cnt[idx])
    below = np.arange(cap)[None, :] < gcnt[:, None]
    assert np.array_equal(gmean[below], mean[idx][below])
    assert np.array_equal(gcov[below], cov[idx][below])
    assert np.isnan(gmean[~below]).all() and np.isnan(gcov[~below]).all()
    assert np.array_equal(gseen, (np.arange(cap) < gcnt.max()).astype(np.int32))


def test_run_equals_steps_and_argument_rules():
    from slamhip._lib import SLAM_ERR_ARG, SlamError
    S = scenario("A")
    sc, steps = S["sc"], S["steps"][:8]
    ctl = np.tile(S["ctl"], (len(steps), 1))
    with _device(sc["n"], sc["cap"], seed=3) as d1, _device(sc["n"], sc["cap"], seed=3) as d2_:
        d1.load_observations([(None, s["obs"]) for s in steps])
        run = d1.run(0, ctl[:5]) + d1.run(5, ctl[5:])
        one = [d2_.step(S["ctl"], None, s["obs"]) for s in steps]
        assert any(r["resampled"] for r in one)
        for k, (a, b) in enumerate(zip(run, one)):
            assert _same(a, b), k
        assert np.array_equal(d1.last_assoc(), d2_.last_assoc())
        assert np.array_equal(d1.get_counts(), d2_.get_counts())
        assert d1.get_counts().max() > 0
        for a, b in zip(d1.get_state() + d1.get_maps() + d1.last_proposal(),
                        d2_.get_state() + d2_.get_maps() + d2_.last_proposal()):
            assert a.tobytes() == b.tobytes()
        t = d1.timing()
        assert t["predict"] > 0 and t["step_end"] > 0
        # the stage calls need control and scan together; the handle refuses ids
        obs0 = steps[0]["obs"]
        for call in (lambda: d1.predict(S["ctl"]), lambda: d1.update(None, obs0),
                     lambda: d1.step(S["ctl"], np.arange(len(obs0)), obs0),
                     lambda: d1.load_observations([(np.arange(len(s["obs"])), s["obs"])
                                                   for s in steps])):
            with pytest.raises(SlamError) as e:
                call()
            assert e.value.code == SLAM_ERR_ARG
        with pytest.raises(SlamError):
            d1.set_counts(np.full(sc["n"], sc["cap"] + 1))    # above the capacity
    with _device(64, 4, record_proposal=False) as quiet:
        quiet.step(S["ctl"], None, steps[0]["obs"])
        with pytest.raises(SlamError):
            quiet.last_proposal()                             # created without record


# ------------------------------------------------------------ 6. frontend
def test_frontend_builds_a_map_from_scans_without_ids():
    """FastSLAM(association="ml_marginal", proposal="measurement") on
    ScanSensor.scan output: every landmark of the best map lies near a true
    one.  The distance is the oracle's own: the float64 restatement's free run
    on the same scans (its own noise stream, as the device draws its own), its
    best map's largest distance to the nearest true landmark, doubled."""
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

    ref = _oracle(n, cap, dict(p_new=P_NEW, noise=NOISE, ess_th=n / 2.0))
    rs = np.random.RandomState(7)
    for sc_ in scans:
        obs = np.array([[o.getDist(), o.getDir(), o.getOrient()] for o in sc_]).reshape(-1, 3)
        out = ref.step(ctl, obs, rs.standard_normal((n, 3)), rs.rand() / n)
    i = out["max_idx"]
    bound = 2.0 * nearest(ref.mean[i, :ref.cnt[i]])
    with FastSLAM(n, cap, association="ml_marginal", proposal="measurement", p_new=P_NEW, q=Q,
                  noise=NOISE, ess_threshold=n / 2.0, seed=1) as slam:
        for sc_ in scans:
            est, cov, (seen, mean, mcov) = slam.step(ctl, sc_)
        seen, mean, mcov = slam.best_map()
        assert slam.step(ctl, (None, np.zeros((0, 3))))[0].shape == (3,)
    held = seen.astype(bool)
    print(f"oracle's best map: {ref.cnt[i]} landmarks, bound {bound:.3g} m; "
          f"device's best map: {held.sum()} landmarks, worst {nearest(mean[held]):.3g} m")
    assert held.sum() >= 1 and np.array_equal(held, np.arange(cap) < held.sum())
    assert np.isfinite(mean[held]).all() and np.isnan(mean[~held]).all()
    assert np.isfinite(est).all() and nearest(mean[held]) <= bound
