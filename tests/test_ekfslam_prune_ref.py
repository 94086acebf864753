"""The EKF-SLAM pruning oracle (tests/ekfslam_prune_ref.py) against itself, CPU
only: the vectorised pass against the plain loop, the empty scan, saturation at
ev_max and INT32_MIN, a NaN mean, removal at the first in-view miss, the removed
state against the np.ix_ gather with a zero tail, and the preconditions and the
claim of DESIGN 11h on the clutter worlds."""
import numpy as np
import pytest

from conftest import ORACLE  # noqa: F401  (puts the oracle on sys.path)

import ekfslam_da_ref as dr
import ekfslam_prune_ref as pr

I32_MIN, I32_MAX = pr.I32_MIN, 2 ** 31 - 1


def random_state(cap, count, seed=0, pose=(1.0, -2.0, 0.7)):
    """A full-size state: ``count`` landmarks within +-12 m, P symmetric with
    distinct entries on the active block, a zero tail."""
    rs = np.random.RandomState(seed)
    n, na = 3 + 3 * cap, 3 + 3 * count
    mu, P = np.zeros(n), np.zeros((n, n))
    mu[:3] = pose
    mu[3:na] = np.column_stack([rs.uniform(-12, 12, (count, 2)), rs.uniform(-3, 3, count)]).ravel()
    A = rs.permutation(na * na).reshape(na, na) + 1.0
    P[:na, :na] = np.tril(A) + np.tril(A, -1).T
    return mu, P


def same_as_loop(mu, P, count, count0, assoc, ev, cfg):
    v = pr.prune_pass(mu, P, count, count0, assoc, ev, cfg)
    mu_l, P_l, count_l, ev_l, removed_l = pr.prune_loop(mu, P, count, count0, assoc, ev, cfg)
    assert v["count"] == count_l and v["removed"] == removed_l == count - count_l
    assert np.array_equal(v["ev"], ev_l) and v["ev"].dtype == np.int32
    assert np.array_equal(v["mu"], mu_l) and np.array_equal(v["P"], P_l)
    return v


@pytest.mark.parametrize("angle", [None, np.deg2rad(80.0), np.deg2rad(120.0)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_vectorised_pass_equals_the_loop_bit_for_bit(angle, seed):
    cap, count, count0 = 24, 20, 17
    rs = np.random.RandomState(100 + seed)
    mu, P = random_state(cap, count, seed)
    cfg = pr.PruneConfig(9.0, view_angle=angle, init=1, hit=2, miss=2, ev_max=4, remove_below=0)
    ev = np.zeros(cap, dtype=np.int32)
    ev[:count] = rs.randint(-1, 5, count)
    assoc = np.array([3, dr.NEW, 11, dr.DROPPED, 0, dr.NEW, dr.NEW], dtype=np.int32)
    v = same_as_loop(mu, P, count, count0, assoc, ev, cfg)
    assert 0 < v["removed"] < count and v["moved"] > 0          # the case exercises a removal
    assert v["in_view"].any() and not v["in_view"].all()


def test_removed_state_is_the_gather_and_the_tail_is_zero():
    cap, count = 12, 11
    mu, P = random_state(cap, count, 3)
    cfg = pr.PruneConfig(1e3, init=0, hit=0, miss=1, ev_max=5, remove_below=0)
    ev = np.zeros(cap, dtype=np.int32)
    ev[[2, 3, 7, 10]] = 1                                      # everything is in view: the others go
    v = same_as_loop(mu, P, count, count, np.empty(0, dtype=np.int32), ev, cfg)
    keep = np.array([2, 3, 7, 10])
    assert np.array_equal(v["keep"], keep) and v["first"] == 0 and v["moved"] == 4
    idx = np.r_[0:3, 9:12, 12:15, 24:27, 33:36]
    assert np.array_equal(pr.gather_index(keep), idx)
    na = idx.size
    assert np.array_equal(v["mu"][:na], mu[idx]) and np.array_equal(v["P"][:na, :na], P[np.ix_(idx, idx)])
    assert not v["mu"][na:].any() and not v["P"][na:].any() and not v["P"][:, na:].any()
    assert v["ev"].tolist() == [0, 0, 0, 0] + [0] * 8 and v["count"] == 4


def test_empty_scan_is_evidence_too():
    cap, count = 6, 5
    mu, P = random_state(cap, count, 4)
    mu[3:5] = mu[:2] + [1.0, 0.0]                              # slot 0 in view
    mu[6:8] = mu[:2] + [50.0, 0.0]                             # slot 1 out of view
    cfg = pr.PruneConfig(9.0, init=1, hit=1, miss=1, ev_max=4, remove_below=0)
    ev = np.array([0, 0, 3, 3, 3, 0], dtype=np.int32)
    v = same_as_loop(mu, P, count, count, np.empty(0, dtype=np.int32), ev, cfg)
    assert 0 not in v["keep"] and 1 in v["keep"]               # in view: 0 - 1 < 0; out of view: unchanged
    assert v["ev"][0] == 0 and v["removed"] >= 1


def test_saturation_at_ev_max_and_int32_min():
    cap = count = 4
    mu, P = random_state(cap, count, 5)
    mu[3:] = np.tile([mu[0] + 1.0, mu[1], 0.0], count)         # all in view
    cfg = pr.PruneConfig(9.0, init=I32_MIN, hit=I32_MAX, miss=I32_MAX, ev_max=I32_MAX,
                         remove_below=I32_MIN)
    ev = np.array([I32_MAX - 1, 5, I32_MIN + 3, I32_MIN], dtype=np.int32)
    v = same_as_loop(mu, P, count, count, np.array([0, 1], dtype=np.int32), ev, cfg)
    assert v["ev"].tolist() == [I32_MAX, I32_MAX, I32_MIN, I32_MIN] and v["removed"] == 0


def test_a_nan_mean_is_not_in_view():
    cap = count = 3
    for angle in (None, np.deg2rad(80.0)):
        mu, P = random_state(cap, count, 6, pose=(0.0, 0.0, np.pi / 2))
        mu[3:5] = [np.nan, 0.0]
        mu[6:8] = [0.0, np.nan]
        mu[9:11] = [0.0, 2.0]                                  # ahead of the robot
        cfg = pr.PruneConfig(9.0, view_angle=angle, init=1, hit=1, miss=1, ev_max=4, remove_below=1)
        ev = np.ones(cap, dtype=np.int32)
        v = pr.prune_pass(mu, P, count, count, np.empty(0, dtype=np.int32), ev, cfg)
        mu_l, P_l, count_l, ev_l, _ = pr.prune_loop(mu, P, count, count, np.empty(0, np.int32), ev, cfg)
        assert v["in_view"].tolist() == [False, False, True] and v["keep"].tolist() == [0, 1]
        assert count_l == 2 and np.array_equal(v["ev"], ev_l)
        assert np.array_equal(v["mu"], mu_l, equal_nan=True) and np.array_equal(v["P"], P_l)
        assert v["margin"] == pytest.approx(7.0 if angle is None else 2.0)    # the NaN slots have none


def test_removal_at_the_first_in_view_miss_with_init_equal_to_remove_below():
    cap, count0 = 5, 2
    mu, P = dr.empty_state(cap)
    cfg = pr.PruneConfig(9.0, init=0, hit=1, miss=1, ev_max=4, remove_below=0)
    lpn = float(np.log(0.1))
    obs = np.array([[3.0, 0.2, 0.1], [4.0, -0.5, 0.3]])
    ev = np.zeros(cap, dtype=np.int32)
    r = pr.observe(mu, P, 0, cap, obs, lpn, ev, cfg)
    assert r["count"] == count0 and r["ev"][:2].tolist() == [0, 0] and r["removed"] == 0
    r2 = pr.observe(r["mu"], r["P"], 2, cap, obs[:1], lpn, r["ev"], cfg)      # slot 1 misses in view
    assert r2["assoc"].tolist() == [0] and r2["keep"].tolist() == [0] and r2["first"] == 1
    assert r2["count"] == 1 and r2["ev"].tolist() == [1, 0, 0, 0, 0] and r2["moved"] == 0
    assert not r2["mu"][6:].any() and not r2["P"][6:].any() and not r2["P"][:, 6:].any()


# ---------------------------------------------------------------- worlds
@pytest.mark.parametrize("name", ["D", "Da", "E"])
def test_world_preconditions(name):
    """What the GPU lockstep tests assert first: float64 and long double decide
    alike from every input (association, in view, evidence, survivors), with
    margins >= 1e-8, and the world removes and moves."""
    r = pr.run(name)
    same, decision, visibility = r.precondition()
    removed, moved, dropped = r.totals()
    print(f"{name}: decisions {r.decisions}, removed {removed}, moved {moved}, dropped {dropped}, "
          f"decision margin {decision:.3g}, visibility margin {visibility:.3g} m, "
          f"final count {r.final_count} of {r.seen} seen, without removal {r.plain}")
    assert same and decision >= 1e-8 and visibility >= 1e-8
    assert removed >= 1 and moved >= 1 and r.free_same
    for s in r.f64:                                            # the chain's own states keep the invariant
        na = 3 + 3 * s["count"]
        assert not s["mu"][na:].any() and not s["P"][na:].any() and not s["P"][:, na:].any()
        assert not s["ev"][s["count"]:].any()


def test_e_crosses_the_tile_edge():
    r = pr.run("E")
    n_act = [3 + 3 * s["count_mid"] for s in r.f64]
    assert min(n_act) < 128 < max(n_act)
    assert any(s["removed"] and 3 + 3 * s["count_mid"] > 128 for s in r.f64)


def test_the_claim_removal_keeps_the_map_from_filling():
    r = pr.run("D")
    assert r.final_count == r.seen == 10 and r.totals()[2] == 0
    assert r.plain["count"] == r.cap == 32 and r.plain["dropped"] >= 1
    small = pr.run("D", 12, False)
    assert small.totals()[2] == 0 and small.plain["dropped"] > 0
