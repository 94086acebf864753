"""EKF-SLAM without ids on the device (slam_ekfslam_observe) against
tests/ekfslam_da_ref.py.

Decisions (every entry of assoc, the count) must equal the oracle's wherever
the oracle alone satisfies the precondition -- float64 and long double decide
alike from the step's input state, smallest finite margin >= 1e-8 -- which each
test asserts first.  Scores, mu and the active block of P must lie within
max(1e-11, 64 x spread) of the long-double restatement, spread being the
float64 oracle's own distance from it (ekfslam_ref.bars' rule; P relative to
max |P| of the result, scores and mu absolute).  After every case the rows and
columns of P and the entries of mu at or beyond n_act are exactly zero.
"""
import contextlib
import functools

import numpy as np
import pytest

from conftest import PKG  # noqa: F401

import ekfslam_da_ref as dr
import ekfslam_ref as er

pytestmark = pytest.mark.gpu

LD = dr.LD


@contextlib.contextmanager
def handle(cap, p_new, **kw):
    from slamhip.ekf import DeviceEKFSLAM
    d = DeviceEKFSLAM(cap, dt=dr.DT, q_robot=dr.Q_ROBOT, noise=dr.NOISE, association="ml",
                      p_new=p_new, record_assoc=True, **kw)
    try:
        yield d
    finally:
        d.close()


def place(d, mu, P, count):
    d.set_state(mu, P)
    d.set_count(count)


def state_with_zero_tail(d):
    """(mu, P, count) of the device; asserts the tail at or beyond n_act is zero."""
    mu, P = d.get_state()
    count = d.count
    na = 3 + 3 * count
    assert d.assoc_info()["n_act"] == na
    assert not mu[na:].any() and not P[na:].any() and not P[:, na:].any()
    return mu, P, count


def embed(mu, P, cap):
    """A state of size 3 + 3 count in a capacity-cap state with a zero tail."""
    n, na = 3 + 3 * cap, mu.size
    mu_f, P_f = np.zeros(n), np.zeros((n, n))
    mu_f[:na], P_f[:na, :na] = mu, P
    return mu_f, P_f


def oracle_pair(mu, P, count, cap, obs, p_new):
    """The float64 and long-double steps from one placed state, with the
    precondition asserted."""
    lpn = float(np.log(p_new))
    f = dr.observe(mu, P, count, cap, obs, lpn)
    l = dr.observe(mu, P, count, cap, obs, lpn, t=LD)
    mg = np.concatenate([f["margin"], l["margin"]])
    mg = mg[np.isfinite(mg)]
    assert np.array_equal(f["assoc"], l["assoc"]) and (mg.size == 0 or mg.min() >= 1e-8), mg
    return f, l


def check_step(d, f, l, spread, what=""):
    """The device's last observe against the oracle step (f float64, l long
    double); returns the errors (scores, P, mu)."""
    assoc = d.last_assoc()
    assert np.array_equal(assoc, f["assoc"]), (what, assoc, f["assoc"])
    mu, P, count = state_with_zero_tail(d)
    assert count == f["count"], (what, count, f["count"])
    info = d.assoc_info()
    assert (info["matched"], info["new"], info["dropped"]) == (
        int((assoc >= 0).sum()), int((assoc == dr.NEW).sum()), int((assoc == dr.DROPPED).sum()))
    err_s = 0.0
    if l["scores"].size:
        sc = d.last_scores()
        assert np.array_equal(np.isnan(sc), np.isnan(l["scores"])), what
        err_s = float(np.abs(np.nan_to_num(sc - l["scores"])).max())
    err_P = float(np.abs(P - l["P"]).max()) / dr.p_scale(l)
    err_mu = float(np.abs(mu - l["mu"]).max())
    print(f"{what}: scores {err_s:.3g} (spread {spread[0]:.3g}), P {err_P:.3g} ({spread[1]:.3g}), "
          f"mu {err_mu:.3g} ({spread[2]:.3g})")
    assert err_s <= dr.bar(spread[0]), (what, err_s, spread[0])
    assert err_P <= dr.bar(spread[1]), (what, err_P, spread[1])
    assert err_mu <= dr.bar(spread[2]), (what, err_mu, spread[2])
    return err_s, err_P, err_mu


# ---------------------------------------------------------------- worlds
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_lockstep_worlds(name):
    """State and count placed from the oracle each step."""
    r = dr.run(name)
    same, margin = r.precondition()
    assert same and margin >= 1e-8
    spread = tuple(np.max([dr.step_spread(f, l) for f, l in zip(r.f64, r.ld)], axis=0))
    with handle(r.cap, r.p_new) as d:
        for i, (f, l) in enumerate(zip(r.f64, r.ld)):
            place(d, f["mu_p"], f["P_p"], f["count0"])
            d.observe(f["obs"])
            check_step(d, f, l, spread, f"{name} step {i}")
            if int((f["assoc"] >= 0).sum()):
                na = 3 + 3 * f["count0"]
                nt = (na + 127) // 128
                assert d.assoc_info()["tiles"] == nt * (nt + 1) // 2


@pytest.mark.parametrize("name", ["A", "C"])
def test_free_run_worlds(name):
    """The device on its own state: every decision the oracle's, the final state
    within the rule, with the spread taken over the run (the two oracle chains'
    largest distance)."""
    r = dr.run(name)
    assert r.precondition()[0]
    assert all(np.array_equal(a, f["assoc"]) for a, f in zip(r.free_assoc, r.f64))
    with handle(r.cap, r.p_new) as d:
        mu0, P0 = dr.empty_state(r.cap)
        place(d, mu0, P0, 0)
        for i, f in enumerate(r.f64):
            assoc = d.step(dr.CONTROL, None, f["obs"])
            assert np.array_equal(assoc, f["assoc"]), (i, assoc, f["assoc"])
            assert d.count == f["count"]
        mu, P, count = state_with_zero_tail(d)
    ref = r.ld_free
    assert count == ref["count"]
    err_P = float(np.abs(P - ref["P"]).max() / np.abs(ref["P"]).max())
    err_mu = float(np.abs(mu - ref["mu"]).max())
    print(f"{name} free run: P {err_P:.3g} (spread {r.free_spread[0]:.3g}), "
          f"mu {err_mu:.3g} (spread {r.free_spread[1]:.3g})")
    assert err_P <= dr.bar(r.free_spread[0]) and err_mu <= dr.bar(r.free_spread[1])


# ----------------------------------------------------------------- edges
@functools.lru_cache(maxsize=None)
def dense_world(n_lm, seed=11):
    """ekfslam_ref.slam_world's dense prior; a principal block of it is a
    smaller world's prior."""
    _, lm, mu, P = er.slam_world(n_lm, seed)
    return lm, mu, P


def dense_case(count, cap, ids, seed=0, n_world=None):
    """A placed state of ``count`` landmarks and observations of ``ids`` from
    near the prior's pose."""
    lm, mu, P = dense_world(n_world or count)
    na = 3 + 3 * count
    mu_f, P_f = embed(mu[:na], P[:na, :na], cap)
    rs = np.random.RandomState(seed)
    obs = er.make_obs(rs, mu[:3] + [0.02, -0.01, 0.005], lm, ids)
    return mu_f, P_f, obs


def full_case(cap, mu, P, count, obs, p_new, what):
    f, l = oracle_pair(mu, P, count, cap, obs, p_new)
    with handle(cap, p_new) as d:
        place(d, mu, P, count)
        d.observe(obs)
        check_step(d, f, l, dr.step_spread(f, l), what)
        info = d.assoc_info()
    return f, info


@pytest.mark.parametrize("k", [1, 40])
def test_empty_map_everything_is_new(k):
    cap = 64
    mu, P = dr.empty_state(cap)
    rs = np.random.RandomState(k)
    obs = np.column_stack([rs.uniform(1, 12, k), rs.uniform(-3, 3, k), rs.uniform(-3, 3, k)])
    f, info = full_case(cap, mu, P, 0, obs, 0.1, f"empty k={k}")
    assert (f["assoc"] == dr.NEW).all() and info["n_act"] == 3 + 3 * k and info["tiles"] == 0


def test_all_matched_is_the_known_id_update_byte_for_byte():
    """No initialisation runs; the update walks the prefix's tiles and equals a
    known-id handle of n_landmarks = count0 given the same state and ids."""
    from slamhip.ekf import DeviceEKFSLAM
    count, cap, ids = 12, 100, [7, 0, 11, 3, 5]
    mu, P, obs = dense_case(count, cap, ids)
    f, l = oracle_pair(mu, P, count, cap, obs, 1e-4)
    assert f["assoc"].tolist() == ids
    na = 3 + 3 * count
    with handle(cap, 1e-4) as d:
        place(d, mu, P, count)
        d.observe(obs)
        check_step(d, f, l, dr.step_spread(f, l), "all matched")
        info = d.assoc_info()
        assert info["new"] == 0 and info["matched"] == 5 and info["n_act"] == na
        assert info["tiles"] == 1 and d.info()["n_tiles"] == 6     # 39 rows of the 303
        assert d.assoc_timing()["init_ms"] == 0.0 and d.assoc_timing()["update_ms"] > 0.0
        mu_a, P_a = d.get_state()
    k = DeviceEKFSLAM(count, dt=dr.DT, q_robot=dr.Q_ROBOT, noise=dr.NOISE)
    try:
        k.set_state(mu[:na], P[:na, :na])
        k.update(ids, obs)
        mu_k, P_k = k.get_state()
    finally:
        k.close()
    assert np.array_equal(mu_a[:na], mu_k) and np.array_equal(P_a[:na, :na], P_k)


def test_full_map_drops_and_leaves_the_state_bit_unchanged():
    count = cap = 8
    mu, P, _ = dense_case(count, cap, [0])
    obs = np.array([[70.0, 0.3, 0.1], [85.0, -2.0, 1.0], [90.0, 2.5, -1.0]])   # beyond every landmark
    f, _ = oracle_pair(mu, P, count, cap, obs, 0.1)
    assert (f["assoc"] == dr.DROPPED).all()
    with handle(cap, 0.1) as d:
        place(d, mu, P, count)
        assert (d.observe(obs) == dr.DROPPED).all()
        mu_d, P_d, c = state_with_zero_tail(d)
        assert c == count and np.array_equal(mu_d, mu) and np.array_equal(P_d, P)
        assert d.assoc_info()["dropped"] == 3 and d.assoc_info()["tiles"] == 0


def test_no_observation_changes_nothing():
    count, cap = 5, 9
    mu, P, _ = dense_case(count, cap, [0])
    with handle(cap, 0.1) as d:
        place(d, mu, P, count)
        assert d.observe(np.empty((0, 3))).size == 0
        mu_d, P_d, c = state_with_zero_tail(d)
        assert c == count and np.array_equal(mu_d, mu) and np.array_equal(P_d, P)


@pytest.mark.parametrize("count", [63, 64, 65, 255, 256, 257, 1024, 1025])
def test_scan_and_assign_sizes(count):
    """Wave, block and assign-stride edges of the scan and the choice: scores
    and decisions only."""
    cap = 1100
    ids = [count - 1, 0, count // 2, min(count - 1, 64), max(0, count - 65)]
    ids = list(dict.fromkeys(ids))
    mu, P, obs = dense_case(count, cap, ids, seed=2, n_world=1025)
    obs = np.vstack([obs, [[70.0, 0.3, 0.1]]])                   # and one that matches nothing
    lpn = float(np.log(1e-4))
    s64, sld = dr.scores(mu, P, count, obs), dr.scores(mu, P, count, obs, t=LD)
    (a64, m64), (ald, mld) = dr.choose(s64, lpn, count, cap), dr.choose(sld, lpn, count, cap)
    assert a64.tolist() == ald.tolist() == ids + [dr.NEW] and min(m64.min(), mld.min()) >= 1e-8
    spread = float(np.abs(s64 - sld).max())
    with handle(cap, 1e-4) as d:
        place(d, mu, P, count)
        assoc = d.observe(obs)
        sc = d.last_scores()
        _, _, c = state_with_zero_tail(d)
    assert np.array_equal(assoc, a64) and c == count + 1
    err = float(np.abs(sc - sld).max())
    print(f"count0={count}: scores {err:.3g} (spread {spread:.3g})")
    assert sc.shape == (len(obs), count) and err <= dr.bar(spread)


@pytest.mark.parametrize("count", [42, 84])
def test_growing_across_a_tile_edge(count):
    """n_act 129 -> 132 (count 42 -> 43) and 255 -> 258: the new landmark's
    rows open a tile row."""
    cap = 100
    ids = [3, count - 1]
    mu, P, obs = dense_case(count, cap, ids, seed=count)
    obs = np.vstack([obs[:1], [[70.0, 0.3, 0.1]], obs[1:]])
    f, info = full_case(cap, mu, P, count, obs, 1e-4, f"grow {count}")
    assert f["assoc"].tolist() == [3, dr.NEW, count - 1]
    assert info["n_act"] == 3 + 3 * (count + 1)
    nt = (3 + 3 * count + 127) // 128
    assert info["tiles"] == nt * (nt + 1) // 2


def test_two_observations_of_one_landmark():
    """The second takes its runner-up or becomes new: a landmark is matched at
    most once per call."""
    count, cap = 10, 20
    mu, P, obs = dense_case(count, cap, [4, 4, 6])
    obs[1] += [0.003, -0.002, 0.001]
    lpn = float(np.log(1e-4))
    raw = dr.scores(mu, P, count, obs)
    assert np.argmax(raw, axis=1).tolist() == [4, 4, 6]
    f, _ = full_case(cap, mu, P, count, obs, 1e-4, "same best slot")
    assert f["assoc"][0] == 4 and f["assoc"][1] != 4 and f["assoc"][2] == 6
    assert f["assoc"][1] == dr.NEW or raw[1, f["assoc"][1]] >= lpn


def test_identical_slots_the_lower_wins():
    count, cap, a, b = 8, 8, 5, 2
    mu, P, obs = dense_case(count, cap, [a])
    ra, rb = slice(3 + 3 * a, 6 + 3 * a), slice(3 + 3 * b, 6 + 3 * b)
    mu[rb] = mu[ra]
    P[rb, :] = P[ra, :]
    P[:, rb] = P[:, ra]
    P[rb, rb] = P[ra, rb] = P[rb, ra] = P[ra, ra]
    assert np.array_equal(P, P.T)
    f = dr.observe(mu, P, count, cap, obs, np.log(1e-4))
    assert f["assoc"].tolist() == [b] and f["scores"][0, a] == f["scores"][0, b]
    with handle(cap, 1e-4) as d:
        place(d, mu, P, count)
        assert d.observe(obs).tolist() == [b]
        sc = d.last_scores()
        assert sc[0, a] == sc[0, b] and np.argmax(sc[0]) == b
        state_with_zero_tail(d)


def test_a_nan_score_never_wins():
    """Slot j holds an indefinite block: det S < 0, the score is NaN."""
    count, cap, j = 8, 12, 3
    mu, P, obs = dense_case(count, cap, [j, 6])
    rj = slice(3 + 3 * j, 6 + 3 * j)
    P[rj, rj] = -1e4 * np.eye(3)
    f = dr.observe(mu, P, count, cap, obs, np.log(1e-4))
    assert np.isnan(f["scores"][:, j]).all() and not np.isnan(np.delete(f["scores"], j, 1)).any()
    assert j not in f["assoc"] and f["assoc"][1] == 6
    with handle(cap, 1e-4) as d:
        place(d, mu, P, count)
        assoc = d.observe(obs)
        sc = d.last_scores()
        assert np.array_equal(np.isnan(sc), np.isnan(f["scores"]))
        assert np.array_equal(assoc, f["assoc"])
        state_with_zero_tail(d)


def test_step_assoc_is_predict_then_observe():
    count, cap = 10, 30
    mu, P, obs = dense_case(count, cap, [2, 9, 5])
    obs = np.vstack([obs, [[70.0, 0.3, 0.1]]])
    ctl = er.CTL
    with handle(cap, 1e-4) as a, handle(cap, 1e-4) as b:
        place(a, mu, P, count)
        place(b, mu, P, count)
        a.predict(ctl)
        ra = a.observe(obs)
        rb = b.step(ctl, None, obs)
        sa, sb = state_with_zero_tail(a), state_with_zero_tail(b)
    assert ra.tolist() == rb.tolist() and ra.tolist()[-1] == dr.NEW
    assert sa[2] == sb[2] == count + 1
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    assert not np.array_equal(sa[0][:3], mu[:3])


def test_update_with_ids_checks_against_the_count():
    from slamhip._lib import SlamError
    count, cap = 5, 9
    mu, P, obs = dense_case(count, cap, [4])
    with handle(cap, 1e-4) as d:
        place(d, mu, P, count)
        with pytest.raises(SlamError, match="out of range"):
            d.update([count], obs)
        d.update([4], obs)
        assert d.assoc_info()["tiles"] == 1
        state_with_zero_tail(d)
