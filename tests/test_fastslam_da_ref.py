"""The associating FastSLAM oracle (tests/fastslam_da_ref.py) against a plain
per-particle loop in matrix form, and the contract's corner cases: exclusion
within a step, a full map, a tie."""
import numpy as np

from conftest import ORACLE  # noqa: F401

import fastslam_da_ref as da
import fastslam_ref as fr

NOISE = (0.1, np.deg2rad(3.0), np.deg2rad(3.0))
Q = np.diag([0.03, 0.03, np.deg2rad(2.0)]) ** 2


def _copy(ref):
    other = da.FSDARef(ref.n, ref.cap, noise=NOISE, ess_th=ref.ess_th)
    other.load(ref)
    other.log_p_new = ref.log_p_new
    return other


def test_vectorised_oracle_equals_the_per_particle_loop():
    n, cap = 16, 6                                   # the map fills: new, matched and dropped
    lm = np.random.RandomState(3).uniform(-12, 12, (40, 2))
    ctl, poses = fr.circle_truth(10)
    rs = np.random.RandomState(5)
    ref = da.FSDARef(n, cap, p_new=0.1, noise=NOISE, ess_th=n / 2.0)
    kinds = set()
    for pose in poses:
        _, obs = fr.observe(pose, lm, 9.0, NOISE, rs)
        u = rs.rand()
        noise = rs.multivariate_normal([0.0, 0.0, 0.0], Q, n)
        out = {"resampled": bool(ref.needs_resample())}
        if out["resampled"]:
            ref._resample(u * (1 / n), out)
        ref._predict(ctl, noise)
        loop = _copy(ref)
        L, assoc, margin = ref.associate_update(obs)
        L2, assoc2 = da.update_loop(loop, obs)
        assert np.array_equal(assoc, assoc2)
        assert np.array_equal(ref.cnt, loop.cnt)
        assert np.allclose(L, L2, rtol=1e-9, atol=1e-9)
        held = np.arange(cap)[None, :] < ref.cnt[:, None]
        assert np.allclose(ref.mean[held], loop.mean[held], rtol=1e-9, atol=1e-9)
        assert np.allclose(ref.cov[held], loop.cov[held], rtol=1e-7, atol=1e-10)
        assert np.isnan(ref.mean[~held]).all() and np.isnan(ref.cov[~held]).all()
        assert margin.shape == assoc.shape and (margin >= 0).all()
        kinds |= {"match"} if (assoc >= 0).any() else set()
        kinds |= {"new"} if (assoc == da.NEW).any() else set()
        kinds |= {"drop"} if (assoc == da.DROPPED).any() else set()
        ref._step_end(L, out)
    assert kinds == {"match", "new", "drop"}, "the run must match, create and drop"


def _one_landmark(n=4, cap=3, p_new=0.1):
    """Every particle at the start pose holding the landmark that a noise-free
    observation z places; returns (ref, z)."""
    ref = da.FSDARef(n, cap, p_new=p_new, noise=NOISE)
    z = np.array([4.0, 0.3, float(fr.wrap(np.array(np.pi / 2 - ref.th[0])))])
    ref.associate_update(z[None, :])
    assert (ref.cnt == 1).all()
    return ref, z


def test_two_observations_of_one_landmark_never_update_the_same_slot():
    ref, z = _one_landmark()
    before = ref.snapshot()
    L, assoc, margin = ref.associate_update(np.stack([z, z]))
    assert (assoc[0] == 0).all()                     # the first matches the landmark
    assert (assoc[1] == da.NEW).all()                # the second may not: it starts slot 1
    assert (ref.cnt == 2).all() and np.isinf(margin[1]).all()
    once = _copy_of(before)
    once.associate_update(z[None, :])
    assert np.array_equal(ref.mean[:, 0], once.mean[:, 0])      # slot 0 was updated once
    assert np.array_equal(ref.cov[:, 0], once.cov[:, 0])
    # a later step sees the slot again
    assert (ref.associate_update(z[None, :])[1][0] == 0).all()


def _copy_of(snap):
    n, cap = snap["mean"].shape[:2]
    ref = da.FSDARef(n, cap, noise=NOISE)
    for k, v in snap.items():
        setattr(ref, k, v.copy())
    return ref


def test_a_full_map_drops_the_observation_and_adds_log_p_new():
    ref, z = _one_landmark(cap=1)
    far = np.array([9.0, -2.0, z[2]])                # nowhere near the landmark held
    before = ref.snapshot()
    ref.use_orient = False
    L, assoc, _ = ref.associate_update(far[None, :])
    assert (assoc == da.DROPPED).all()
    assert np.array_equal(L, np.full(ref.n, ref.log_p_new))
    assert np.array_equal(ref.cnt, before["cnt"])
    assert ref.mean.tobytes() == before["mean"].tobytes()
    assert ref.cov.tobytes() == before["cov"].tobytes()


def test_a_tie_takes_the_lowest_slot():
    ref, z = _one_landmark(cap=4)
    for j in (1, 2):                                 # exact copies of slot 0
        ref.mean[:, j], ref.cov[:, j] = ref.mean[:, 0], ref.cov[:, 0]
    ref.cnt[:] = 3
    pre = ref.snapshot()
    L, assoc, margin = ref.associate_update(z[None, :])
    assert (assoc[0] == 0).all() and (margin[0] == 0).all()
    assert (da.update_loop(_copy_of(pre), z[None, :])[1][0] == 0).all()
    # the first of two equal observations takes slot 0; slots 1 and 2 then tie
    two = _copy_of(pre).associate_update(np.stack([z, z]))[1]
    assert (two[0] == 0).all() and (two[1] == 1).all()
