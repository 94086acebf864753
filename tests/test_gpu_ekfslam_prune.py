"""EKF-SLAM landmark evidence and removal on the device (slam_ekfslam_set_pruning,
slam_ekfslam_remove) against tests/ekfslam_prune_ref.py.

The compaction is a permutation of stored numbers: mu, P and the evidence after
a removal must equal the host's np.ix_ gather bit for bit, with an exactly zero
tail.  Decisions (assoc, count, evidence, removed) must equal the oracle's
wherever the oracle alone satisfies the preconditions -- float64 and long double
decide alike from the step's input, decision and visibility margins >= 1e-8 --
which each world test asserts first.  mu and P of a step are held to
ekfslam_da_ref.bar of the step's own float64 against long-double spread.
"""
import contextlib

import numpy as np
import pytest

from conftest import PKG  # noqa: F401

import ekfslam_da_ref as dr
import ekfslam_prune_ref as pr
import ekfslam_ref as er

pytestmark = pytest.mark.gpu

# the kernels' own sizes (csrc/eks_prune.hpp): the row pass's strip is 16 columns and its
# batch 64 rows, the column pass's chunk 2,048 columns, the evidence kernel's chunk 1,024 slots
EV_CHUNK = 1024


@contextlib.contextmanager
def handle(cap, p_new=0.1, **kw):
    from slamhip.ekf import DeviceEKFSLAM
    d = DeviceEKFSLAM(cap, dt=dr.DT, q_robot=dr.Q_ROBOT, noise=dr.NOISE, association="ml",
                      p_new=p_new, **kw)
    try:
        yield d
    finally:
        d.close()


def place(d, mu, P, count, ev=None):
    d.set_state(mu, P)
    d.set_count(count)
    if ev is not None:
        d.set_evidence(ev)


def state_with_zero_tail(d):
    mu, P = d.get_state()
    count = d.count
    na = 3 + 3 * count
    assert d.assoc_info()["n_act"] == na
    assert not mu[na:].any() and not P[na:].any() and not P[:, na:].any()
    return mu, P, count


def distinct_state(cap, seed=0):
    """count = cap; mu and the lower triangle of P hold distinct numbers."""
    n = 3 + 3 * cap
    rs = np.random.RandomState(seed)
    mu = rs.permutation(n) + 0.25
    A = rs.permutation(n * n).reshape(n, n) + 1.0
    return mu, np.tril(A) + np.tril(A, -1).T


def patterns(cap):
    """slot 0 only, the last only, one in the middle, every second slot, a run of
    five, all but one, all."""
    mid = cap // 2
    out = {"first": [0], "last": [cap - 1], "middle": [mid], "every second": list(range(0, cap, 2)),
           "run of five": list(range(cap // 3, min(cap // 3 + 5, cap))),
           "all but one": [j for j in range(cap) if j != mid], "all": list(range(cap))}
    return out


def check_removed(d, mu, P, cap, gone, what):
    keep = np.setdiff1d(np.arange(cap), gone)
    mu_x, P_x = pr.remove_slots(mu, P, keep)
    mu_d, P_d, count = state_with_zero_tail(d)
    assert count == keep.size, (what, count)
    assert np.array_equal(mu_d, mu_x), what
    bad = np.argwhere(P_d != P_x)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())
    info = d.prune_info()
    first = int(min(gone))
    assert (info["count_before"], info["removed"], info["first"]) == (cap, len(gone), first), (what, info)
    assert info["moved"] == int((keep > first).sum()), (what, info)
    return keep


# cap 4: n = 15; 43: n = 132, one slot past the 128 edge; 96: n = 291; the
# neighbours (n = 3 + 3 cap takes every third size) of the row pass's strip (16
# columns: n = 15, 18) and batch (64 rows: n = 63, 66, 69), of the column
# pass's chunk (2,048 columns: n = 2,046 .. 2,055; a removal of slot 0 starts
# the chunks at column 3)
@pytest.mark.parametrize("cap", [1, 4, 5, 9, 20, 21, 22, 43, 96, 681, 682, 683, 684])
def test_compaction_alone(cap):
    mu, P = distinct_state(cap, cap)
    with handle(cap, prune=dict(view_range=5.0)) as d:
        for what, gone in patterns(cap).items():
            if not gone:                                        # cap 1 has no "all but one"
                continue
            place(d, mu, P, cap, np.arange(cap) + 7)
            d.remove(gone)
            keep = check_removed(d, mu, P, cap, gone, f"cap {cap} {what}")
            ev = d.evidence()
            assert np.array_equal(ev[:keep.size], keep + 7) and not ev[keep.size:].any(), what


def test_compaction_of_several_strips_and_chunks():
    """cap 700: n = 2,103, P is 35 MB; 132 strips, two chunks a row."""
    cap = 700
    mu, P = distinct_state(cap, 1)
    with handle(cap) as d:                                      # a handle that does not prune
        for what, gone in patterns(cap).items():
            if what in ("first", "every second", "run of five", "all but one"):
                place(d, mu, P, cap)
                d.remove(gone)
                check_removed(d, mu, P, cap, gone, f"cap {cap} {what}")


@pytest.mark.parametrize("cap", [EV_CHUNK - 1, EV_CHUNK, EV_CHUNK + 1, 2 * EV_CHUNK + 77])
def test_scan_across_the_evidence_kernels_chunks(cap):
    """The keep flags' scan at the 1,024-slot chunk edge: the source map is seen
    through mu and the evidence (P stays zero: 75 MB of it would only cost time)."""
    n = 3 + 3 * cap
    mu = np.random.RandomState(cap).permutation(n) + 0.5
    rs = np.random.RandomState(cap + 1)
    with handle(cap, prune=dict(view_range=5.0)) as d:
        for gone in ([cap - 1], [0, cap - 1], np.flatnonzero(rs.rand(cap) < 0.4).tolist(),
                     list(range(1, cap)), [EV_CHUNK - 2]):
            d.set_state(mu)
            d.set_count(cap)
            d.set_evidence(np.arange(cap) - 5)
            d.remove(gone)
            keep = np.setdiff1d(np.arange(cap), gone)
            mu_d = d.get_state(with_cov=False)
            idx = pr.gather_index(keep)
            assert d.count == keep.size
            assert np.array_equal(mu_d[:idx.size], mu[idx]) and not mu_d[idx.size:].any()
            ev = d.evidence()
            assert np.array_equal(ev[:keep.size], keep - 5) and not ev[keep.size:].any()
            info = d.prune_info()
            assert (info["removed"], info["first"], info["moved"]) == (
                len(gone), min(gone), int((keep > min(gone)).sum()))


def test_two_removals_equal_the_combined_one():
    cap = 96
    mu, P = distinct_state(cap, 2)
    a, b = [3, 4, 50, 95], [0, 10, 11, 49, 51, 94]              # b in the original numbering
    keep_a = np.setdiff1d(np.arange(cap), a)
    b_after_a = np.flatnonzero(np.isin(keep_a, b))
    with handle(cap) as d, handle(cap) as e:
        place(d, mu, P, cap)
        d.remove(a)
        d.remove(b_after_a)
        place(e, mu, P, cap)
        e.remove(sorted(a + b))
        sd, se = state_with_zero_tail(d), state_with_zero_tail(e)
    assert sd[2] == se[2] == cap - 10
    assert np.array_equal(sd[0], se[0]) and np.array_equal(sd[1], se[1])
    mu_x, P_x = pr.remove_slots(mu, P, np.setdiff1d(np.arange(cap), a + b))
    assert np.array_equal(sd[0], mu_x) and np.array_equal(sd[1], P_x)


# ---------------------------------------------- a compacted handle is a fresh one
@pytest.mark.parametrize("count,gone,ids", [(20, [3, 7, 8], [0, 2, 5, 16]),
                                            (50, [0, 9, 10, 11, 30, 44, 45, 46, 47, 49], [1, 20, 39]),
                                            (43, [42], [0, 41])])
def test_a_compacted_handle_behaves_like_a_fresh_one(count, gone, ids):
    """After remove, one observe gives the bytes of the same observe on a fresh
    handle placed at the gathered state (n_act 153 -> 123 and 132 -> 129 cross
    the 128-row tile edge)."""
    cap = count + 6
    _, lm, mu_w, P_w = er.slam_world(count, 11)
    na = 3 + 3 * count
    mu, P = np.zeros(3 + 3 * cap), np.zeros((3 + 3 * cap, 3 + 3 * cap))
    mu[:na], P[:na, :na] = mu_w, P_w
    keep = np.setdiff1d(np.arange(count), gone)
    obs = er.make_obs(np.random.RandomState(5), mu[:3] + [0.02, -0.01, 0.005], lm[keep], ids)
    obs = np.vstack([obs, [[70.0, 0.3, 0.1]]])                  # and one that starts a landmark
    mu_x, P_x = pr.remove_slots(mu, P, keep)
    with handle(cap, 1e-4) as d, handle(cap, 1e-4) as f:
        place(d, mu, P, count)
        d.remove(gone)
        place(f, mu_x, P_x, keep.size)
        a_d, a_f = d.observe(obs), f.observe(obs)
        sd, sf = state_with_zero_tail(d), state_with_zero_tail(f)
    assert a_d.tolist() == a_f.tolist() and a_d[-1] == dr.NEW and (a_d[:-1] >= 0).all(), a_d
    assert sd[2] == sf[2] == keep.size + 1
    assert np.array_equal(sd[0], sf[0]) and np.array_equal(sd[1], sf[1])


# ---------------------------------------------------------------- worlds
def assert_preconditions(r):
    same, decision, visibility = r.precondition()
    removed, moved, _ = r.totals()
    assert same and decision >= 1e-8 and visibility >= 1e-8, (same, decision, visibility)
    assert removed >= 1 and moved >= 1


def prune_kw(r):
    return r.cfg.front_end(r.angle)


@pytest.mark.parametrize("name", ["D", "Da", "E"])
def test_lockstep_worlds(name):
    """The oracle's predicted state and evidence placed each step."""
    r = pr.run(name)
    assert_preconditions(r)
    spread = tuple(np.max([dr.step_spread(f, l) for f, l in zip(r.f64, r.ld)], axis=0))
    worst = [0.0, 0.0]
    with handle(r.cap, r.p_new, prune=prune_kw(r)) as d:
        for i, (f, l) in enumerate(zip(r.f64, r.ld)):
            place(d, f["mu_p"], f["P_p"], f["count0"], f["ev0"])
            assoc = d.observe(f["obs"])
            assert np.array_equal(assoc, f["assoc"]), (i, assoc, f["assoc"])
            assert np.array_equal(d.last_assoc(), f["assoc"])
            mu, P, count = state_with_zero_tail(d)
            info, ainfo = d.prune_info(), d.assoc_info()
            assert count == f["count"] == ainfo["count"], (i, count, f["count"])
            assert np.array_equal(d.evidence(), f["ev"]), (i, d.evidence(), f["ev"])
            assert (info["count_before"], info["removed"], info["moved"], info["first"]) == (
                f["count_mid"], f["removed"], f["moved"], f["first"]), (i, info)
            assert (ainfo["count0"], ainfo["new"]) == (f["count0"], int((assoc == dr.NEW).sum()))
            err_P = float(np.abs(P - l["P"]).max()) / dr.p_scale(l)
            err_mu = float(np.abs(mu - l["mu"]).max())
            worst = [max(worst[0], err_P), max(worst[1], err_mu)]
            assert err_P <= dr.bar(spread[1]), (i, err_P, spread[1])
            assert err_mu <= dr.bar(spread[2]), (i, err_mu, spread[2])
    print(f"{name}: P {worst[0]:.3g} (spread {spread[1]:.3g}), mu {worst[1]:.3g} (spread {spread[2]:.3g})")


def test_free_run_of_d():
    """The device on its own state: every decision the oracle's, the count 10 at
    the end, the state within the rule of the two oracle chains' distance."""
    r = pr.run("D")
    assert_preconditions(r)
    assert r.free_same
    with handle(r.cap, r.p_new, prune=prune_kw(r)) as d:
        mu0, P0 = dr.empty_state(r.cap)
        place(d, mu0, P0, 0)
        for i, f in enumerate(r.f64):
            assoc = d.step(dr.CONTROL, None, f["obs"])
            assert np.array_equal(assoc, f["assoc"]), (i, assoc, f["assoc"])
            assert d.count == f["count"] and d.prune_info()["removed"] == f["removed"], i
            assert np.array_equal(d.evidence(), f["ev"]), i
        mu, P, count = state_with_zero_tail(d)
    ref = r.ld_free
    assert count == ref["count"] == 10
    err_P = float(np.abs(P - ref["P"]).max() / np.abs(ref["P"]).max())
    err_mu = float(np.abs(mu - ref["mu"]).max())
    print(f"D free run: P {err_P:.3g} (spread {r.free_spread[0]:.3g}), "
          f"mu {err_mu:.3g} (spread {r.free_spread[1]:.3g})")
    assert err_P <= dr.bar(r.free_spread[0]) and err_mu <= dr.bar(r.free_spread[1])


def test_off_is_off():
    """Until the first removal a pruning handle's state is the bytes of one that
    does not prune; at the first removal it is the host's gather of that state
    by the oracle's survivors.  Pruning set and cleared again leaves no trace."""
    r = pr.run("D")
    assert_preconditions(r)
    first = next(i for i, f in enumerate(r.f64) if f["removed"])
    with handle(r.cap, r.p_new, prune=prune_kw(r)) as a, handle(r.cap, r.p_new) as b, \
            handle(r.cap, r.p_new, prune=prune_kw(r)) as c:
        c.set_pruning(None)
        mu0, P0 = dr.empty_state(r.cap)
        for d in (a, b, c):
            place(d, mu0, P0, 0)
        for i, f in enumerate(r.f64):
            ra = a.step(dr.CONTROL, None, f["obs"]) if i <= first else None
            rb, rc = b.step(dr.CONTROL, None, f["obs"]), c.step(dr.CONTROL, None, f["obs"])
            sb, sc = state_with_zero_tail(b), state_with_zero_tail(c)
            assert np.array_equal(rb, rc) and sb[2] == sc[2]
            assert np.array_equal(sb[0], sc[0]) and np.array_equal(sb[1], sc[1]), i
            if i > first:
                continue
            sa = state_with_zero_tail(a)
            assert np.array_equal(ra, rb), i
            if i < first:
                assert a.prune_info()["removed"] == 0 and sa[2] == sb[2]
                assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]), i
            else:
                assert a.prune_info()["removed"] == f["removed"] and f["count_mid"] == sb[2]
                mu_x, P_x = pr.remove_slots(sb[0], sb[1], f["keep"])
                assert sa[2] == f["keep"].size
                assert np.array_equal(sa[0], mu_x) and np.array_equal(sa[1], P_x)
        from slamhip._lib import SlamError
        with pytest.raises(SlamError, match="pruning is off"):
            c.evidence()


@pytest.mark.parametrize("cap", [32, 12])
def test_the_claim(cap):
    """D's scans: with removal the map ends at the 10 landmarks seen and nothing
    is dropped; without, it fills and sightings are dropped."""
    r = pr.run("D", cap, cap == 32)
    with handle(cap, r.p_new, prune=prune_kw(r)) as a, handle(cap, r.p_new) as b:
        mu0, P0 = dr.empty_state(cap)
        dropped = [0, 0]
        for q, d in enumerate((a, b)):
            place(d, mu0, P0, 0)
            for z in r.scans:
                d.step(dr.CONTROL, None, z)
                dropped[q] += d.assoc_info()["dropped"]
        counts = (a.count, b.count)
    print(f"cap {cap}: count {counts[0]} / {counts[1]}, dropped {dropped[0]} / {dropped[1]}")
    assert counts[0] == 10 and dropped[0] == 0
    assert counts[1] == cap and dropped[1] >= 1


def test_front_end():
    from ekf_slam import EKFSLAM
    r = pr.run("D")
    kw = dict(dt=dr.DT, q_robot=dr.Q_ROBOT, noise=dr.NOISE, p_new=r.p_new, prune=prune_kw(r))
    with EKFSLAM(r.cap, x0=dr.X0, p0=np.diag(dr.P0_RR), **kw) as s, \
            handle(r.cap, r.p_new, prune=prune_kw(r)) as d:
        mu0, P0 = dr.empty_state(r.cap)
        place(d, mu0, P0, 0)
        for z in r.scans:
            _, _, (mean, cov) = s.step(dr.CONTROL, (None, z))
            d.step(dr.CONTROL, None, z)
        m_d, c_d = d.landmarks()
        assert s.count == d.count == 10 and mean.shape == (10, 3)
        assert np.array_equal(mean, m_d) and np.array_equal(cov, c_d)
        m_s, c_s = s.map()
        assert np.array_equal(m_s, m_d) and np.array_equal(c_s, c_d)
    with pytest.raises(ValueError, match="prune"):
        EKFSLAM(10, association=None, prune=dict(view_range=7.2))


# ------------------------------------------------------------------- the API
def test_modes_evidence_accessors_and_argument_errors():
    from slamhip._lib import SlamError
    cap, count = 8, 5
    mu, P = distinct_state(cap, 3)
    na = 3 + 3 * count
    mu[na:], P[na:], P[:, na:] = 0.0, 0.0, 0.0
    mu[:3] = [0.0, 0.0, np.pi / 2]
    mu[3:na] = np.array([[0, 2, 0], [0, 50, 0], [1, 3, 0], [0, -2, 0], [2, 2, 0]], float).ravel()
    with handle(cap) as d:
        place(d, mu, P, count)
        for call in (d.evidence, lambda: d.set_evidence(np.zeros(cap))):
            with pytest.raises(SlamError, match="pruning is off"):
                call()
        for bad in ([1, 1], [2, 1], [count], [-1]):
            with pytest.raises(SlamError, match="strictly increasing"):
                d.remove(bad)
        d.remove([])
        assert d.count == count and d.prune_info()["count_before"] == 0
        d.set_pruning(9.0, init=2, ev_max=3)
        assert d.evidence().tolist() == [2] * count + [0] * (cap - count)     # turned on: init
        d.set_evidence([5, 6, 7, 8, 9, 99, 99, 99])
        d.set_pruning(9.0, view_angle=np.deg2rad(80.0), init=0, hit=1, miss=6, ev_max=9)
        assert d.evidence().tolist() == [5, 6, 7, 8, 9, 0, 0, 0]              # only the rule changed
        # an empty scan is evidence too: slots 0, 2, 4 lie in the fan ahead, slot 3
        # behind the robot, slot 1 out of range
        assert d.observe(np.empty((0, 3))).size == 0
        assert d.evidence().tolist() == [6, 1, 8, 3, 0, 0, 0, 0] and d.count == 4
        info = d.prune_info()
        assert (info["count_before"], info["removed"], info["moved"], info["first"]) == (5, 1, 4, 0)
        assert info["evidence_ms"] > 0.0 and info["compact_ms"] > 0.0
        mu_x, P_x = pr.remove_slots(mu, P, np.array([1, 2, 3, 4]))
        mu_d, P_d, _ = state_with_zero_tail(d)
        assert np.array_equal(mu_d, mu_x) and np.array_equal(P_d, P_x)
        d.set_count(3)
        assert d.evidence().tolist() == [0, 0, 0, 0, 0, 0, 0, 0]              # set_count: init (0 now)
        d.set_pruning(None)
        with pytest.raises(SlamError, match="pruning is off"):
            d.evidence()
        d.set_pruning(9.0, init=4, ev_max=4)
        assert d.evidence().tolist() == [4, 4, 4, 0, 0, 0, 0, 0]
        with pytest.raises(SlamError, match="ev_max"):
            d.set_pruning(9.0, init=5, ev_max=4)
        # slam_ekfslam_update with ids leaves the evidence alone
        _, lm, mu_w, P_w = er.slam_world(3, 11)
        mu_s, P_s = np.zeros_like(mu), np.zeros_like(P)
        mu_s[:12], P_s[:12, :12] = mu_w, P_w
        place(d, mu_s, P_s, 3, [1, 2, 3, 0, 0, 0, 0, 0])
        d.update([1], er.make_obs(np.random.RandomState(0), mu_w[:3], lm, [1]))
        assert d.evidence().tolist() == [1, 2, 3, 0, 0, 0, 0, 0] and d.count == 3
        assert not np.array_equal(d.get_state(with_cov=False), mu_s)
    from slamhip.ekf import DeviceEKFSLAM
    k = DeviceEKFSLAM(4, dt=dr.DT, q_robot=dr.Q_ROBOT, noise=dr.NOISE)
    try:
        with pytest.raises(ValueError, match="association"):
            k.set_pruning(9.0)
        cfg = __import__("slamhip.fastslam", fromlist=["prune_config"]).prune_config(9.0)
        import ctypes as C
        from slamhip._lib import SLAM_ERR_ARG
        assert k._lib.slam_ekfslam_set_pruning(k._h, C.byref(cfg)) == SLAM_ERR_ARG
        assert k._lib.slam_ekfslam_remove(k._h, 0, None) == SLAM_ERR_ARG
    finally:
        k.close()
