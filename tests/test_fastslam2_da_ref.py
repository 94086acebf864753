"""The oracle of FastSLAM 2.0 without ids (tests/fastslam2_da_ref.py) against
itself: its score against the 1.0 score where the pose covariance is zero, the
vectorised form against a plain per-particle loop in matrix form, a world in
which the association cannot go wrong against the known-id 2.0 oracle, and the
property the proposal is for -- a larger effective sample size than the 1.0
filter that associates the same scans.
"""
import numpy as np

from conftest import ORACLE  # noqa: F401  (puts the oracle on sys.path)

import fastslam2_da_ref as d2
import fastslam2_ref as f2
import fastslam_da_ref as da
import fastslam_ref as fr

NOISE = (0.1, np.deg2rad(3.0), np.deg2rad(3.0))
Q = np.diag([0.2, 0.2, np.deg2rad(5.0)]) ** 2
LD = np.longdouble


def _err_mean(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b) / (1 + np.abs(b)))) if a.size else 0.0


def _err_cov(a, b):
    """[..., m] rows against each row's largest entry."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    if not a.size:
        return 0.0
    return float(np.max(np.abs(a - b) / np.max(np.abs(b), axis=-1, keepdims=True)))


def _held(a, cnt):
    return a[np.arange(a.shape[1])[None, :] < cnt[:, None]]


# ------------------------------------------------- a. the score at Sigma = 0
def test_score_without_pose_covariance_is_the_fastslam_1_score():
    rs = np.random.RandomState(2)
    n = 500
    x, y, th = 10 + rs.normal(0, 0.5, n), rs.normal(0, 0.5, n), np.pi / 2 + rs.normal(0, 0.2, n)
    mx, my = rs.uniform(-12, 12, n), rs.uniform(-12, 12, n)
    a = rs.normal(0, 0.3, (n, 2, 2))
    P = a @ np.swapaxes(a, -1, -2) + 0.01 * np.eye(2)
    pxx, pxy, pyy = P[:, 0, 0], P[:, 0, 1], P[:, 1, 1]
    d, phi = rs.uniform(1, 15, n), rs.uniform(-np.pi, np.pi, n)
    R0, R1 = fr.scan_r(d, NOISE[0], NOISE[1])
    c, s = np.cos(np.pi / 2 - th), np.sin(np.pi / 2 - th)
    zero = tuple(np.zeros(n) for _ in range(6))
    l0 = d2.score_terms(x, y, c, s, zero, mx, my, pxx, pxy, pyy, d, phi, R0, R1)[0]
    want = fr.update_landmark(x, y, c, s, mx, my, pxx, pxy, pyy, d, phi, R0, R1)[5]
    ln2pi = np.log(2 * np.pi)
    err = np.max(np.abs((l0 - ln2pi) - (want - ln2pi)) / (1 + np.abs(want - ln2pi)))
    print(f"score at Sigma = 0 against the 1.0 score: {err:.3g}")
    assert err <= 1e-12
    # a pose covariance only lowers the peak and widens the tails: S grows
    sig = tuple(np.full(n, v) for v in (Q[0, 0], 0.0, 0.0, Q[1, 1], 0.0, Q[2, 2]))
    det0 = d2.score_terms(x, y, c, s, zero, mx, my, pxx, pxy, pyy, d, phi, R0, R1)[3]
    det1 = d2.score_terms(x, y, c, s, sig, mx, my, pxx, pxy, pyy, d, phi, R0, R1)[3]
    assert (det1 > det0).all()


# ----------------------------------- b. vectorised against the plain loop
def _copy(ref):
    other = d2.FS2DARef(ref.n, ref.cap, ref.Q, noise=NOISE, ess_th=ref.ess_th)
    other.load(ref)
    other.log_p_new = ref.log_p_new
    return other


def test_vectorised_oracle_equals_the_per_particle_loop():
    n, cap, steps = 64, 8, 6                          # the map fills: new, matched and dropped
    lm = np.random.RandomState(3).uniform(-12, 12, (40, 2))
    ctl, poses = fr.circle_truth(steps)
    rs = np.random.RandomState(5)
    ref = d2.FS2DARef(n, cap, Q, p_new=0.1, noise=NOISE, ess_th=n / 2.0)
    kinds, worst = set(), dict(mu=0.0, sigma=0.0, L=0.0, pose=0.0, mean=0.0, cov=0.0)
    for pose in poses:
        _, obs = fr.observe(pose, lm, 9.0, NOISE, rs)
        u = rs.rand()
        xi = rs.standard_normal((n, 3))
        if ref.needs_resample():
            ref._resample(u * (1 / n), {})
        loop = _copy(ref)
        out = ref.step(ctl, obs, xi, u * (1 / n))
        assert not out["resampled"]                   # the resampling was done above
        mus, sigmas, L2, assoc2 = d2.step_loop(loop, ctl, obs, xi)
        assert np.array_equal(out["assoc"], assoc2)
        assert np.array_equal(ref.cnt, loop.cnt)
        sig2 = np.stack([sigmas[:, i, j] for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))],
                        axis=1)
        err = dict(mu=_err_mean(out["mu"], mus), sigma=_err_cov(out["sigma"], sig2),
                   L=_err_mean(out["L"], L2),
                   pose=_err_mean(np.column_stack([ref.x, ref.y, ref.th]),
                                  np.column_stack([loop.x, loop.y, loop.th])),
                   mean=_err_mean(_held(ref.mean, ref.cnt), _held(loop.mean, ref.cnt)),
                   cov=_err_cov(_held(ref.cov, ref.cnt), _held(loop.cov, ref.cnt)))
        for k, e in err.items():
            worst[k] = max(worst[k], e)
        held = np.arange(cap)[None, :] < ref.cnt[:, None]
        assert np.isnan(ref.mean[~held]).all() and np.isnan(ref.cov[~held]).all()
        assert out["margin"].shape == out["assoc"].shape and (out["margin"] >= 0).all()
        a = out["assoc"]
        kinds |= ({"match"} if (a >= 0).any() else set()) | ({"new"} if (a == d2.NEW).any() else set())
        kinds |= {"drop"} if (a == d2.DROPPED).any() else set()
    print(f"vectorised against the loop, worst: {worst}")
    assert all(e <= 1e-12 for e in worst.values()), worst
    assert kinds == {"match", "new", "drop"}, "the run must match, create and drop"


# ------------------------- c. an unambiguous world: the known-id 2.0 filter
def _separated_world(seed, count=6, apart=6.0):
    """``count`` landmarks drawn uniformly in (-14, 14)^2, each kept only if it
    lies at least ``apart`` from those before it."""
    rs = np.random.RandomState(seed)
    pts = []
    while len(pts) < count:
        p = rs.uniform(-14, 14, 2)
        if all(np.hypot(*(p - q)) >= apart for q in pts):
            pts.append(p)
    return np.array(pts)


def test_well_separated_landmarks_reproduce_the_known_id_filter():
    """Six landmarks at least 6 m apart, p_new = 1e-4: every particle's choices
    are the true landmarks' slots, so the filter is the known-id 2.0 filter on
    a permuted map.  Two things keep the association beyond doubt.  The scan
    noise drawn is a fifth of what the filters model (R's bearing entry is
    (d sin r_dir)^2, so at 9 m a bearing weighs little and p_new = 1e-4 is a
    gate near four sigma of the modelled noise: an honest 3.7-sigma range draw
    starts a new landmark in some particles).  And in this world (seed 4 of
    the sampler below, 12 m sensor range) the landmarks in view never share a
    range; the smallest decision margin of the run is 5.5 in log likelihood."""
    n, steps = 200, 60
    lm = _separated_world(4)
    dist = np.hypot(lm[:, None, 0] - lm[None, :, 0], lm[:, None, 1] - lm[None, :, 1])
    assert dist[np.triu_indices(6, 1)].min() >= 6.0
    sim = (0.02, np.deg2rad(1.0), np.deg2rad(1.0))
    ctl, poses = fr.circle_truth(steps)
    rs = np.random.RandomState(5)
    kw = dict(noise=NOISE, ess_th=n / 2.0)
    ml = d2.FS2DARef(n, 6, Q, p_new=1e-4, **kw)
    known = f2.FS2Ref(n, 6, Q, **kw)
    slot = {}                                         # landmark id -> the slot it was created in
    worst = dict(mu=0.0, sigma=0.0, pose=0.0, w=0.0, mean=0.0, cov=0.0, Lconst=0.0)
    matched = 0
    for pose in poses:
        ids, obs = fr.observe(pose, lm, 12.0, sim, rs)
        ofs = rs.rand() * (1 / n)
        xi = rs.standard_normal((n, 3))
        want = []
        for j in ids:
            if int(j) in slot:
                want.append(slot[int(j)])
            else:
                slot[int(j)] = len(slot)
                want.append(d2.NEW)
        a = ml.step(ctl, obs, xi, ofs)
        b = known.step(ctl, ids, obs, xi, ofs)
        assert np.array_equal(a["assoc"], np.tile(np.array(want, dtype=np.int32)[:, None], (1, n)))
        assert a["resampled"] == b["resampled"]
        matched += sum(1 for v in want if v >= 0)
        seen_ids = np.array(sorted(slot), dtype=np.int64)
        slots = np.array([slot[int(j)] for j in seen_ids], dtype=np.int64)
        assert (ml.cnt == len(slot)).all()
        dL = np.asarray(a["L"] - b["L"], dtype=np.float64)
        err = dict(mu=_err_mean(a["mu"], b["mu"]), sigma=_err_cov(a["sigma"], b["sigma"]),
                   pose=_err_mean(np.column_stack([ml.x, ml.y, ml.th]),
                                  np.column_stack([known.x, known.y, known.th])),
                   w=float(np.max(np.abs(ml.w - known.w) / known.w)),
                   mean=_err_mean(ml.mean[:, slots], known.mean[:, seen_ids]),
                   cov=_err_cov(ml.cov[:, slots], known.cov[:, seen_ids]),
                   Lconst=float(np.max(np.abs(dL - dL[0])) / (1 + abs(dL[0]))))
        for k, e in err.items():
            worst[k] = max(worst[k], e)
    print(f"against the known-id oracle, worst: {worst}; {matched} matched observations")
    assert matched > 100 and len(slot) >= 3
    assert all(e <= 1e-12 for e in worst.values()), worst


# ---------------------------------------- d. what the proposal is for
def test_the_proposal_keeps_a_larger_effective_sample_size_without_ids():
    """NP = 1000, 60 steps, stream 5, 12 landmarks in 9 m range, ESS_TH = NP / 2,
    p_new = 0.1, capacity 24: the same controls, scans, offsets and normals for
    both associating filters (the 1.0 filter's motion noise is xi @ F, F^T F =
    Q).  Asserted as a plain inequality of the medians of ESS / NP."""
    n, nl, steps, cap = 1000, 12, 60, 24
    lm = np.random.RandomState(3).uniform(-15, 15, (nl, 2))
    ctl, poses = fr.circle_truth(steps)
    rs = np.random.RandomState(5)
    kw = dict(p_new=0.1, noise=NOISE, ess_th=n / 2.0)
    two, one = d2.FS2DARef(n, cap, Q, **kw), da.FSDARef(n, cap, **kw)
    F = np.linalg.cholesky(Q).T
    ess = {1: [], 2: []}
    for pose in poses:
        _, obs = fr.observe(pose, lm, 9.0, NOISE, rs)
        ofs = rs.rand() * (1 / n)
        xi = rs.standard_normal((n, 3))
        ess[2].append(two.step(ctl, obs, xi, ofs)["ess"])
        ess[1].append(one.step(ctl, obs, xi @ F, ofs)["ess"])
    m1, m2 = np.median(ess[1]) / n, np.median(ess[2]) / n
    print(f"median ESS / NP without ids: 2.0 {m2:.3f}, 1.0 {m1:.3f}; "
          f"final counts 2.0 {two.cnt.min()}..{two.cnt.max()}, 1.0 {one.cnt.min()}..{one.cnt.max()}")
    assert m2 > m1
