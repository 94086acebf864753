"""FastSLAM oracle, CPU side: the scalar 2 x 2 landmark update of
tests/fastslam_ref.py against the generic matrix form, and the initialisation
against theory."""
import numpy as np

from conftest import ORACLE  # noqa: F401  (puts the oracle on sys.path)

import fastslam_ref as fr


def _random_case(rs):
    pose = np.array([rs.uniform(-5, 5), rs.uniform(-5, 5), rs.uniform(-np.pi, np.pi)])
    mean = pose[:2] + rs.uniform(1.0, 8.0) * np.array([np.cos(a := rs.uniform(-np.pi, np.pi)), np.sin(a)])
    a = rs.uniform(-1, 1, (2, 2))
    P = a @ a.T + 0.05 * np.eye(2)                        # positive definite
    d = np.hypot(*(mean - pose[:2])) * rs.uniform(0.9, 1.1)
    psi = np.pi / 2 - pose[2]
    c, s = np.cos(psi), np.sin(psi)
    dx, dy = mean - pose[:2]
    phi = np.arctan2(s * dx + c * dy, c * dx - s * dy) + rs.uniform(-0.1, 0.1)
    return pose, mean, P, d, phi


def test_scalar_update_equals_the_matrix_form():
    rs = np.random.RandomState(11)
    for _ in range(200):
        pose, mean, P, d, phi = _random_case(rs)
        R0, R1 = fr.scan_r(d, 0.1, np.deg2rad(3.0))
        psi = np.pi / 2 - pose[2]
        one = lambda v: np.array([v])                     # noqa: E731
        r = fr.update_landmark(one(pose[0]), one(pose[1]), one(np.cos(psi)), one(np.sin(psi)),
                               one(mean[0]), one(mean[1]), one(P[0, 0]), one(P[0, 1]), one(P[1, 1]),
                               d, phi, R0, R1)
        m2, P2, dl = fr.update_landmark_generic(pose, mean, P, (d, phi), np.diag([R0, R1]))
        got_m = np.array([r[0][0], r[1][0]])
        got_P = np.array([[r[2][0], r[3][0]], [r[3][0], r[4][0]]])
        scale = max(1.0, np.abs(P).max(), np.abs(mean).max())
        assert np.abs(got_m - m2).max() <= 1e-12 * scale
        assert np.abs(got_P - P2).max() <= 1e-12 * scale
        assert abs(r[5][0] - dl) <= 1e-12 * max(1.0, abs(dl))


def test_initialisation_then_zero_innovation_halves_the_covariance():
    """A landmark initialised from an observation has P0 = A R A^T with A the
    inverse of H at that landmark, so H P0 H^T = R; a second identical
    observation (zero innovation) then gives K = P0 H^T (2 R)^-1 and
    P1 = P0 - K (2 R) K^T = P0 / 2, the mean unchanged, and a log weight of
    -ln det(2 R) / 2."""
    rs = np.random.RandomState(12)
    for _ in range(100):
        pose = np.array([rs.uniform(-5, 5), rs.uniform(-5, 5), rs.uniform(-np.pi, np.pi)])
        d, phi = rs.uniform(0.5, 12.0), rs.uniform(-np.pi, np.pi)
        R0, R1 = fr.scan_r(d, 0.1, np.deg2rad(3.0))
        psi = np.pi / 2 - pose[2]
        one = lambda v: np.array([v])                     # noqa: E731
        x, y, c, s = one(pose[0]), one(pose[1]), one(np.cos(psi)), one(np.sin(psi))
        mx, my, pxx, pxy, pyy = fr.init_landmark(x, y, c, s, d, phi, R0, R1)
        assert np.isclose(np.hypot(mx - x, my - y), d, rtol=1e-13)
        r = fr.update_landmark(x, y, c, s, mx, my, pxx, pxy, pyy, d, phi, R0, R1)
        big = max(pxx[0], pyy[0])
        assert abs(r[0][0] - mx[0]) <= 1e-9 * (1 + abs(mx[0]))
        assert abs(r[1][0] - my[0]) <= 1e-9 * (1 + abs(my[0]))
        for got, p0 in zip(r[2:5], (pxx, pxy, pyy)):
            assert abs(got[0] - p0[0] / 2) <= 1e-9 * big
        assert np.isclose(r[5][0], -np.log(4 * R0 * R1) / 2, rtol=1e-9, atol=1e-9)


def test_log_domain_weights_survive_where_the_product_overflows():
    """k = 300 density factors of ~1e3 each overflow fp64 as a product; the
    shifted exponent of their log sum does not."""
    L = np.full(4, 300 * np.log(1e3)) + np.array([0.0, -1.0, -2.0, -700.0])
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(L)).all()
    w = np.exp(L - L.max())
    assert w[0] == 1.0 and np.isfinite(w).all() and w[3] > 0


def test_reference_step_counts_seen_landmarks_and_keeps_unobserved_ones():
    f = fr.FSRef(50, 4, ess_th=25.0)
    rs = np.random.RandomState(0)
    ctl, poses = fr.circle_truth(3)
    lm = np.array([[11.0, 3.0], [8.0, -2.0], [-30.0, 0.0], [12.0, 1.0]])
    for k, pose in enumerate(poses):
        ids, obs = fr.observe(pose, lm, 9.0, (0.1, 0.05, 0.05), rs)
        assert list(ids) == [0, 1, 3]
        before = f.mean[:, 2].copy()
        out = f.step(ctl, ids, obs, rs.standard_normal((50, 3)) * 0.01,
                     rs.rand() / 50 if f.needs_resample() else None)
        assert np.array_equal(before, f.mean[:, 2], equal_nan=True)      # never observed
        assert np.isclose(f.w.sum(), 1.0) and out["max_idx"] == int(np.argmax(f.w))
    assert list(f.seen) == [True, True, False, True]
    assert np.isfinite(f.mean[:, [0, 1, 3]]).all() and np.isnan(f.mean[:, 2]).all()
