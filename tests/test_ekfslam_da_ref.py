"""The restatement of EKF-SLAM without ids (tests/ekfslam_da_ref.py) checked on
the CPU: the vectorised score against the plain loop, the inverse measurement
model and its Jacobians, the covariance staying symmetric positive definite,
and the precondition of every decision-parity test of
tests/test_gpu_ekfslam_assoc.py -- float64 and long double decide alike from
every step's input state, with the smallest finite margin >= 1e-8."""
import numpy as np
import pytest

from conftest import ORACLE  # noqa: F401  (puts the oracle on sys.path)

import ekf_oracle as eo
import ekfslam_da_ref as dr
import ekfslam_ref as er


def test_vectorised_scores_equal_the_plain_loop():
    _, _, mu, P = er.slam_world(9, 5)
    rs = np.random.RandomState(0)
    xr = mu[:3] + [0.05, -0.02, 0.01]
    lm = mu[3:].reshape(-1, 3)
    obs = er.make_obs(rs, xr, lm, [4, 0, 7]).tolist() + [[25.0, 1.0, -2.0]]
    a = dr.scores(mu, P, 9, obs)
    b = dr.scores_loop(mu, P, 9, obs)
    assert a.shape == (4, 9)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    ld = dr.scores(mu, P, 9, obs, t=dr.LD)
    assert np.abs(a - ld).max() <= 1e-11 * np.abs(b).max()
    # the observations of landmarks 4, 0, 7 pick them
    assoc, margin = dr.choose(a, np.log(1e-4), 9, 9)
    assert assoc.tolist() == [4, 0, 7, dr.DROPPED] and np.all(margin > 1e-8)


def test_choose_rules():
    inf = np.inf
    l = np.array([[1.0, 3.0, 3.0, np.nan],        # tie: the lowest slot
                  [0.0, 9.0, 2.0, np.nan],        # slot 1 is taken: the runner-up
                  [-5.0, 9.0, 9.0, np.nan],       # best left is below log_p_new: new
                  [np.nan, 9.0, 9.0, np.nan],     # NaN never wins, nothing left: new -> dropped
                  [5.0, 9.0, 9.0, np.nan]])
    assoc, margin = dr.choose(l, -1.0, 4, 5)
    assert assoc.tolist() == [1, 2, dr.NEW, dr.DROPPED, 0]
    assert margin[0] == 0.0 and margin[1] == 2.0 and margin[2] == 4.0 and margin[3] == inf
    assoc, _ = dr.choose(np.empty((3, 0)), -1.0, 0, 2)
    assert assoc.tolist() == [dr.NEW, dr.NEW, dr.DROPPED]


def test_inverse_model_round_trips_and_its_jacobians():
    rs = np.random.RandomState(1)
    for _ in range(20):
        xr = np.array([rs.uniform(-5, 5), rs.uniform(-5, 5), rs.uniform(-3, 3)])
        z = np.array([rs.uniform(0.5, 12), rs.uniform(-3, 3), rs.uniform(-3, 3)])
        lm, _, _ = dr.inverse_model(xr, z)
        back = eo.scan_predict(xr, lm)
        d = back - z
        d[1:] = dr.wrap(d[1:], np.float64)
        assert np.abs(d).max() < 1e-13
        Gr, Gz = dr.init_jacobians(xr, z)
        h = 1e-6
        for G, base, which in ((Gr, xr, 0), (Gz, z, 1)):
            for q in range(3):
                dp, dm = base.copy(), base.copy()
                dp[q] += h
                dm[q] -= h
                gp = dr.inverse_model(*((dp, z) if which == 0 else (xr, dp)))[0]
                gm = dr.inverse_model(*((dm, z) if which == 0 else (xr, dm)))[0]
                diff = gp - gm
                diff[2] = dr.wrap(diff[2], np.float64)
                assert np.abs(diff / (2 * h) - G[:, q]).max() < 5e-8


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_worlds_satisfy_the_precondition(name):
    r = dr.run(name)
    same, margin = r.precondition()
    assert same and margin >= 1e-8, (same, margin)
    assert all(np.array_equal(a, f["assoc"]) for a, f in zip(r.free_assoc, r.f64))
    last = r.f64[-1]
    na = 3 + 3 * last["count"]
    P = last["P"]
    assert np.array_equal(P, P.T) and np.linalg.eigvalsh(P[:na, :na]).min() > 0
    assert not P[na:].any() and not P[:, na:].any() and not last["mu"][na:].any()
    if name == "B":
        assert last["count"] == r.cap and any((f["assoc"] == dr.DROPPED).any() for f in r.f64)
    if name == "C":
        assert max(len(z) for z in r.scans) == 40
        assert any(3 + 3 * f["count0"] <= 128 < 3 + 3 * f["count"] for f in r.f64)
