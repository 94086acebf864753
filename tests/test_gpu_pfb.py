"""Particle-filter ensemble (slam_pfb_*, slamhip.pf_batch) on the GPU (-m gpu).

Inputs: filter b draws from RandomState(1000 + seed0 + b), in the order
landmarks uniform(-10, 10, (NL, 2)) [-> per-filter parameters], then per step
[random_sample() if the oracle resamples] -> process noise -> observation
noise.  The oracle (oracle/pf_oracle.py) runs once per input set and is shared.

Bars
  * against the oracle (tests 1, 6): those of test_step_covariance_vs_oracle --
    resampled / max_idx / resample_next equal, x_est rtol 1e-6, cov rtol 1e-6
    atol 1e-12, ess 1e-9 relative; final weights weights_match(rtol 1e-9,
    floor 1e-290) (a multi-step trajectory);
  * against NumPy on the device's own weights (tests 2, 3): bit-exact;
  * against a single slam_pf handle (tests 4, 5): bit-identical state, weights,
    weight_sum, max_val, max_idx, x_est, resampled; ess 1e-10 relative and cov
    rtol 1e-8 (their summation order is each kernel's own);
  * run against run / step (tests 6, 7): bit-identical records and state.
Every test asserts the oracle's resample count it relies on.
"""
import functools

import numpy as np
import pytest

from conftest import heavy_weights, weights_match

import pf_oracle as po

pytestmark = pytest.mark.gpu

REC_FIELDS = ("x_est", "cov", "max_val", "ess", "weight_sum", "max_idx", "resampled",
              "resample_next", "status", "ess_near")


@pytest.fixture(scope="module")
def pfb():
    from slamhip import pf_batch
    return pf_batch


@pytest.fixture(scope="module")
def dpf():
    from slamhip import pf
    return pf


@functools.lru_cache(maxsize=None)
def trajectory(B, NP, NL, steps, motion, seed0, ess_frac, hetero=False):
    """The oracle's lockstep trajectory of B filters: per filter its parameters,
    per step the inputs (u, noise, z), the oracle's outputs and its post-step
    ESS / weights.  ess_frac: ESS_TH = NP * ess_frac."""
    filters = []
    for b in range(B):
        rs = np.random.RandomState(1000 + seed0 + b)
        lm = rs.uniform(-10, 10, (NL, 2))
        p = po.PFParams(n_particles=NP, landmarks=lm, motion=motion)
        p.ess_th = NP * ess_frac
        if hetero:                                    # per-filter r, x0, ESS threshold
            p.r = np.diag(rs.uniform(0.2, 0.4, 2)) ** 2
            p.x0 = p.x0 + rs.normal(0.0, 0.2, 3)
            p.ess_th = NP * rs.uniform(0.4, 0.6)
        orc, world = po.PFOracle(p), po.PFWorld(p)
        rows = []
        for _ in range(steps):
            xt = world.advance().copy()
            u = float(rs.random_sample()) if orc.needs_resample() else None
            if motion == "linear":
                noise = rs.multivariate_normal([0.0, 0.0, 0.0], p.q, NP)
            else:
                noise = rs.standard_normal((NP, 3))
            z = po.to_robot_frame(xt, lm) + rs.multivariate_normal([0.0, 0.0], p.r, NL)
            out = orc.step(z, noise, None if u is None else u * p.np_recip)
            ess = po.ess_of(orc.w)
            rows.append(dict(u=u, noise=noise, z=z, out=out, ess=ess, truth=xt,
                             resample_next=ess < p.ess_th, w=orc.w.copy(),
                             state=(orc.x.copy(), orc.y.copy(), orc.th.copy())))
        filters.append(dict(p=p, lm=lm, rows=rows,
                            resamples=sum(bool(r["out"]["resampled"]) for r in rows),
                            margin=min(abs(r["ess"] - p.ess_th) / p.ess_th for r in rows)))
    return filters


def make_ensemble(pfb, fl, **kw):
    p0 = fl[0]["p"]
    return pfb.BatchParticleFilter(
        len(fl), p0.np, np.array([f["lm"] for f in fl]), motion=p0.motion,
        r=np.array([f["p"].r for f in fl]), x0=np.array([f["p"].x0 for f in fl]),
        ess_threshold=np.array([f["p"].ess_th for f in fl]), **kw)


def step_inputs(fl, k):
    u = np.array([np.nan if f["rows"][k]["u"] is None else f["rows"][k]["u"] for f in fl])
    return (np.array([f["rows"][k]["z"] for f in fl]),
            np.array([f["rows"][k]["noise"] for f in fl]), u)


def check_against_oracle(fl, k, outs):
    for b, (f, rd) in enumerate(zip(fl, outs)):
        row = f["rows"][k]
        ro = row["out"]
        assert rd["resampled"] == bool(ro["resampled"]), (k, b)
        assert rd["max_idx"] == ro["max_idx"], (k, b)
        np.testing.assert_allclose(rd["x_est"], ro["x_est"], rtol=1e-6)
        np.testing.assert_allclose(rd["cov"], ro["cov"], rtol=1e-6, atol=1e-12)
        assert abs(rd["ess"] - row["ess"]) <= 1e-9 * row["ess"], (k, b)
        assert rd["resample_next"] == bool(row["resample_next"]), (k, b)
        assert rd["status"] == 0, (k, b)


def lockstep(pfb, fl, likelihood):
    p0 = fl[0]["p"]
    steps = len(fl[0]["rows"])
    with make_ensemble(pfb, fl, likelihood=likelihood) as e:
        for k in range(steps):
            z, noise, u = step_inputs(fl, k)
            outs = e.step((p0.vel, p0.omega), z, noise, u)
            check_against_oracle(fl, k, outs)
        w = e.get_state()[3]
    for b, f in enumerate(fl):
        weights_match(w[b], f["rows"][-1]["w"], rtol=1e-9, floor=1e-290)


# --------------------------------------------------------------- 1. oracle
@pytest.mark.parametrize("likelihood", ["product", "logsum"])
def test_lockstep_linear_vs_oracle(pfb, likelihood):
    fl = trajectory(6, 500, 20, 25, "linear", 0, 0.01)
    assert all(f["resamples"] >= 3 for f in fl) and min(f["margin"] for f in fl) > 1e-6
    lockstep(pfb, fl, likelihood)


def test_lockstep_velocity_vs_oracle(pfb):
    fl = trajectory(6, 1000, 20, 25, "velocity", 10, 0.01)
    assert all(f["resamples"] >= 3 for f in fl) and min(f["margin"] for f in fl) > 1e-6
    lockstep(pfb, fl, "product")


# ---------------------------------------------------------------- 2. numpy
def numpy_indices(w, u):
    n = w.size
    return np.searchsorted(np.cumsum(w), np.arange(0.0, 1.0, 1 / n)[:n] + u / n, "left")


def check_numpy_on_device_weights(e, outs):
    n = e.n
    w_un, s = e.get_weights_raw()
    x, y, th, w = e.get_state()
    for b, rd in enumerate(outs):
        assert s[b] == np.sum(w_un[b].reshape(1, n)), b
        assert rd["weight_sum"] == s[b]
        ref = w_un[b] / s[b]
        ref[np.isnan(ref)] = 1 / n
        np.testing.assert_array_equal(w[b], ref)
        assert rd["max_val"] == np.max(w[b]) and rd["max_idx"] == int(np.argmax(w[b])), b
    return x, y, th, w


@pytest.mark.parametrize("n", [7, 129, 8192])
def test_numpy_order_on_device_weights(pfb, n):
    """np.sum, the division, max / first argmax and the exact resampling
    indices against NumPy on the device's own weights: NP below 8 (the plain
    loop), one leaf with a remainder, and the full buffer (64 leaves, 16 passes
    of the block)."""
    fl = trajectory(3, n, 5, 12, "linear", 30 + n, 0.5)
    assert all(f["resamples"] >= 8 for f in fl) and min(f["margin"] for f in fl) > 1e-6
    p0 = fl[0]["p"]
    with make_ensemble(pfb, fl) as e:
        pending = None
        for k in range(12):
            z, noise, u = step_inputs(fl, k)
            outs = e.step((p0.vel, p0.omega), z, noise, u)
            check_against_oracle(fl, k, outs)
            x, y, th, w = check_numpy_on_device_weights(e, outs)
            if pending is not None:                 # the gathered particles, moved (:129-140, :166)
                for b, (idx, px, py, pth) in pending.items():
                    assert outs[b]["resampled"]
                    gx, gy, gt = po.motion_linear(px[idx], py[idx], pth[idx], p0.dt, p0.vel, p0.omega)
                    np.testing.assert_allclose(x[b], gx + noise[b][:, 0], rtol=0, atol=1e-12)
                    np.testing.assert_allclose(y[b], gy + noise[b][:, 1], rtol=0, atol=1e-12)
                    np.testing.assert_allclose(th[b], gt + noise[b][:, 2], rtol=0, atol=1e-12)
            pending = None
            if k + 1 < 12 and any(o["resample_next"] for o in outs):
                un = np.array([f["rows"][k + 1]["u"] if f["rows"][k + 1]["u"] is not None else 0.5
                               for f in fl])
                idx = e.resample_indices(un)
                pending = {}
                for b, o in enumerate(outs):
                    np.testing.assert_array_equal(idx[b], numpy_indices(w[b], un[b]))
                    if o["resample_next"]:
                        pending[b] = (idx[b], x[b], y[b], th[b])


def test_single_particle_filters_and_the_nan_rule(pfb):
    fl = trajectory(3, 1, 5, 12, "linear", 31, 0.5)
    assert all(f["resamples"] == 0 for f in fl)
    p0 = fl[0]["p"]
    with make_ensemble(pfb, fl) as e:
        for k in range(12):
            z, noise, u = step_inputs(fl, k)
            outs = e.step((p0.vel, p0.omega), z, noise, u)
            check_against_oracle(fl, k, outs)
            check_numpy_on_device_weights(e, outs)
            assert all(o["max_val"] == 1.0 and o["max_idx"] == 0 and not o["resampled"] for o in outs)
        # an observation so far away that the likelihood underflows: 0 / 0 -> 1/NP
        z, noise, u = step_inputs(fl, 11)
        outs = e.step((p0.vel, p0.omega), z + 1e3, noise, u)
        w_un, s = e.get_weights_raw()
        assert np.all(w_un == 0.0) and np.all(s == 0.0)
        assert np.all(e.get_state()[3] == 1.0)
        assert all(o["max_val"] == 1.0 and not o["resampled"] and not o["resample_next"] for o in outs)


# ------------------------------------------------- 3. heavy and tied weights
def test_heavy_weights_indices_bit_exact(pfb):
    n, B = 8192, 3
    ws = []
    for b in range(B):
        w = heavy_weights(np.random.RandomState(77 + b), n, zero_frac=0.5)
        w[:64] = 0.0
        ws.append(w / np.sum(w.reshape(1, n)))
    ws = np.array(ws)
    u = np.array([0.25, 0.5, 0.875])
    ref = np.array([numpy_indices(ws[b], u[b]) for b in range(B)])
    assert ref.max() < n                                   # no IndexError in the reference
    with pfb.BatchParticleFilter(B, n, np.zeros((1, 2))) as e:
        e.set_state(w=ws)
        assert not e.resample_next.any()               # ESS ~ 350 > NP / 100
        np.testing.assert_array_equal(e.resample_indices(u), ref)
        np.testing.assert_array_equal(e.get_state()[3], ws)


def test_uniform_and_concentrated_weights_and_first_argmax(pfb):
    n, B = 1000, 3
    ws = np.full((B, n), 1 / n)
    ws[1] = 0.0
    ws[1, -1] = 1.0                                        # all weight on the last particle
    w2 = heavy_weights(np.random.RandomState(5), n)
    ws[2] = w2 / np.sum(w2.reshape(1, n))
    u = np.array([0.5, 0.5, 0.3])
    ref = np.array([numpy_indices(ws[b], u[b]) for b in range(B)])
    assert ref.max() < n and np.all(ref[1] == n - 1)
    lm = np.random.RandomState(6).uniform(-10, 10, (4, 2))
    p = po.PFParams(n_particles=n, landmarks=lm)
    with pfb.BatchParticleFilter(B, n, lm) as e:
        e.set_state(w=ws)
        np.testing.assert_array_equal(e.resample_next, [False, True, False])
        np.testing.assert_array_equal(e.resample_indices(u), ref)
        # every particle of a filter in the same state, no noise: all weights
        # tie after the step, and the first index is the argmax
        z = np.tile(po.to_robot_frame(p.x0, lm), (B, 1, 1))
        e.set_resample_next([0, 1, 0])
        outs = e.step((p.vel, p.omega), z, np.zeros((B, n, 3)), u)
        w = e.get_state()[3]
        assert [o["resampled"] for o in outs] == [False, True, False]
        assert outs[0]["max_idx"] == 0 and outs[1]["max_idx"] == 0
        assert np.all(w[0] == w[0][0]) and np.all(w[1] == w[1][0])
        assert outs[2]["max_idx"] == int(np.argmax(w[2]))


# ------------------------------------------------ 4. equal to a single handle
def compare_with_single(rb, rs, tag):
    for f in ("max_val", "weight_sum", "max_idx", "resampled", "resample_next"):
        assert rb[f] == rs[f], (tag, f, rb[f], rs[f])
    np.testing.assert_array_equal(rb["x_est"], rs["x_est"])
    assert abs(rb["ess"] - rs["ess"]) <= 1e-10 * rs["ess"], tag
    np.testing.assert_allclose(rb["cov"], rs["cov"], rtol=1e-8)


def test_member_equals_single_handle_host_noise(pfb, dpf):
    fl = trajectory(6, 500, 20, 25, "linear", 0, 0.01)
    assert all(f["resamples"] >= 3 for f in fl)
    p0 = fl[0]["p"]
    singles = [dpf.DeviceParticleFilter(p0.np, f["lm"]) for f in fl]
    try:
        with make_ensemble(pfb, fl) as e:
            for k in range(25):
                z, noise, u = step_inputs(fl, k)
                outs = e.step((p0.vel, p0.omega), z, noise, u)
                state = e.get_state()
                for b, d in enumerate(singles):
                    rs = d.step((p0.vel, p0.omega), z[b], noise[b], u[b])
                    compare_with_single(outs[b], rs, (k, b))
                    for a, c in zip(state, d.get_state()):
                        np.testing.assert_array_equal(a[b], c)
    finally:
        for d in singles:
            d.close()


# ------------------------------------------------- 5. device RNG, reproducible
def test_device_rng_member_is_a_stand_alone_filter(pfb, dpf):
    B, n, nl, steps = 5, 1000, 20, 16
    fl = trajectory(B, n, nl, steps, "velocity", 50, 0.01)
    p0 = fl[0]["p"]
    lms = np.array([f["lm"] for f in fl])
    zs = np.array([[f["rows"][k]["z"] for f in fl] for k in range(steps)])     # [steps][B][NL][2]
    ctl = np.tile([p0.vel, p0.omega], (steps, 1))
    seeds = np.arange(7, 7 + B)
    with pfb.BatchParticleFilter(B, n, lms, motion="velocity", seed=seeds) as e:
        e.load_observations(zs)
        out = e.run(0, ctl)
        state = e.get_state()
    assert sum(out[k][b]["resampled"] for k in range(steps) for b in range(B)) >= 1
    for b in range(B):
        with dpf.DeviceParticleFilter(n, lms[b], motion="velocity", seed=int(seeds[b])) as d:
            d.load_observations(zs[:, b])
            ref = d.run(0, ctl)
            sref = d.get_state()
        assert not any(r["ess_near"] for r in ref)         # a flagged step would void the comparison
        for k in range(steps):
            compare_with_single(out[k][b], ref[k], (k, b))
        for a, c in zip(state, sref):
            np.testing.assert_array_equal(a[b], c)
        err = np.array([np.hypot(*(out[k][b]["x_est"][:2] - fl[b]["rows"][k]["truth"][:2]))
                        for k in range(steps)])
        assert np.all(np.isfinite(err)) and np.median(err) < 0.5


# --------------------------------- 6. more filters than fit at once, heterogeneous
def records_equal(a, b):
    for f in REC_FIELDS:
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)


def test_many_heterogeneous_filters(pfb):
    B, n, nl, steps = 300, 64, 3, 6
    fl = trajectory(B, n, nl, steps, "linear", 99, 0.5, True)
    assert all(f["resamples"] >= 1 for f in fl) and min(f["margin"] for f in fl) > 1e-6
    p0 = fl[0]["p"]
    with make_ensemble(pfb, fl) as e:
        for k in range(steps):
            z, noise, u = step_inputs(fl, k)
            check_against_oracle(fl, k, e.step((p0.vel, p0.omega), z, noise, u))
        w = e.get_state()[3]
    for b, f in enumerate(fl):
        weights_match(w[b], f["rows"][-1]["w"], rtol=1e-9, floor=1e-290)
    # run has no noise input: two identical ensembles (device RNG) give the same
    # bits, and one run of 6 steps equals six runs of 1
    zs = np.array([[f["rows"][k]["z"] for f in fl] for k in range(steps)])
    ctl = np.tile([p0.vel, p0.omega], (steps, 1))
    got = []
    for split in (False, False, True):
        with make_ensemble(pfb, fl, seed=np.arange(B) + 3) as e:
            e.load_observations(zs)
            if split:
                rec = np.concatenate([e.run(k, ctl[k:k + 1]).records.copy() for k in range(steps)])
            else:
                rec = e.run(0, ctl).records.copy()
            got.append((rec, e.get_state()))
    assert got[0][0]["resampled"].sum() >= 1
    for rec, state in got[1:]:
        records_equal(rec, got[0][0])
        for a, c in zip(state, got[0][1]):
            np.testing.assert_array_equal(a, c)


# ---------------------------------------------------- 7. run == repeated step
def test_run_equals_repeated_step_device_rng(pfb):
    B, n, nl, steps = 4, 500, 20, 8
    fl = trajectory(B, n, nl, steps, "linear", 70, 0.01)
    p0 = fl[0]["p"]
    zs = np.array([[f["rows"][k]["z"] for f in fl] for k in range(steps)])
    ctl = np.tile([p0.vel, p0.omega], (steps, 1))
    with make_ensemble(pfb, fl, seed=np.arange(B) + 21) as e, \
            make_ensemble(pfb, fl, seed=np.arange(B) + 21) as twin:
        e.load_observations(zs)
        out = e.run(0, ctl)
        for k in range(steps):
            outs = twin.step(ctl[k], zs[k])
            for b in range(B):
                for f in REC_FIELDS:
                    np.testing.assert_array_equal(out[k][b][f], outs[b][f], err_msg=f"{k} {b} {f}")
        for a, c in zip(e.get_state(), twin.get_state()):
            np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(e.resample_next, twin.resample_next)


# ------------------------------------------------------------------ 8. timing
@pytest.mark.parametrize("steps", [4, 16])
def test_a_run_is_one_launch(pfb, steps):
    B, n, nl = 8, 200, 4
    rs = np.random.RandomState(3)
    lm = rs.uniform(-10, 10, (nl, 2))
    p = po.PFParams(n_particles=n, landmarks=lm)
    zs = np.tile(po.to_robot_frame(p.x0, lm), (steps, B, 1, 1))
    with pfb.BatchParticleFilter(B, n, lm, seed=np.arange(B)) as e:
        e.load_observations(zs)
        out = e.run(0, np.tile([p.vel, p.omega], (steps, 1)))
        ms, launches = e.timing()
    assert launches == 1 and ms > 0.0
    assert len(out) == steps and len(out[0]) == B and out.records.shape == (steps, B)
