"""The NumPy restatement of the landmark map (tests/graph_map_ref.py) on its
own: the mean is the minimiser it claims to be, the map moves with the poses,
a single observation gives itself, and the CPU experiment of DESIGN 8.7."""
import numpy as np
import pytest

import graph_map_ref as mr


def _random_case(seed, n_poses=7, n_landmarks=3, n_halves=17):
    rs = np.random.RandomState(seed)
    poses = np.column_stack([rs.uniform(-10, 10, n_poses), rs.uniform(-10, 10, n_poses),
                             rs.uniform(-np.pi, np.pi, n_poses)])
    p = rs.randint(0, n_poses, n_halves)
    halves = np.column_stack([p, p, rs.randint(0, n_landmarks, n_halves), rs.uniform(2, 15, n_halves),
                              rs.uniform(-np.pi, np.pi, n_halves), rs.uniform(-np.pi, np.pi, n_halves)])
    return poses, halves.astype(np.float64)


def test_mean_is_the_stationary_point():
    """The gradient of sum_k (L_k - m)^T W_k (L_k - m) vanishes at mean_l
    (central differences)."""
    poses, halves = _random_case(1)
    mean, _, count, _, _ = mr.landmark_map(halves, 3, poses)
    for l in range(3):
        terms = [mr.half_terms(h, poses) for h in halves if int(h[2]) == l]
        assert count[l] == len(terms) >= 2

        def cost(m):
            return sum((L - m) @ (W @ (L - m)) for L, _, W in terms)

        scale = cost(mean[l] + 1.0)                 # the cost one metre away
        for axis in np.eye(2):
            g = (cost(mean[l] + 1e-4 * axis) - cost(mean[l] - 1e-4 * axis)) / 2e-4
            assert abs(g) < 1e-7 * scale, (l, g, scale)


def test_equivariant_under_a_rigid_motion():
    poses, halves = _random_case(2)
    mean, cov, count, chi2, half = mr.landmark_map(halves, 3, poses)
    phi, t = 0.7, np.array([3.0, -2.0])
    R = np.array([[np.cos(phi), -np.sin(phi)], [np.sin(phi), np.cos(phi)]])
    moved = poses.copy()
    moved[:, 0:2] = poses[:, 0:2] @ R.T + t
    moved[:, 2] = poses[:, 2] + phi
    mean2, cov2, count2, chi22, half2 = mr.landmark_map(halves, 3, moved)
    np.testing.assert_array_equal(count, count2)
    np.testing.assert_allclose(mean2, mean @ R.T + t, rtol=0, atol=1e-12)
    np.testing.assert_allclose(cov2, R @ cov @ R.T, rtol=0, atol=1e-12 * np.abs(cov).max())
    np.testing.assert_allclose(chi22, chi2, rtol=1e-10)
    np.testing.assert_allclose(half2, half, rtol=1e-9, atol=1e-12)


def test_single_observation_and_unseen_landmark():
    poses, halves = _random_case(3)
    one = halves[:1].copy()
    one[0, 2] = 1
    ignored = halves[1:2].copy()
    ignored[0, 2] = 7                                # outside [0, 3)
    mean, cov, count, chi2, half = mr.landmark_map(np.concatenate([one, ignored]), 3, poses)
    L, C, _ = mr.half_terms(one[0], poses)
    np.testing.assert_array_equal(count, [0, 1, 0])
    np.testing.assert_array_equal(mean[1], L)
    np.testing.assert_allclose(cov[1], C, rtol=1e-13)
    assert chi2[1] == 0.0 and half[0] == 0.0 and np.isnan(half[1])
    for l in (0, 2):
        assert np.isnan(mean[l]).all() and np.isnan(cov[l]).all() and np.isnan(chi2[l])


# seed: map RMS at the dead-reckoned start, at the optimised poses, at the true
# poses (m), and sum chi2 / dof at the optimised poses (DESIGN 8.7's table)
TABLE = {0: (0.663, 0.357, 0.125, 1.13), 5: (1.075, 0.218, 0.109, 1.16), 6: (0.857, 0.271, 0.112, 1.18)}


@pytest.mark.parametrize("seed", sorted(TABLE))
def test_cpu_experiment(seed):
    """72 poses, 16 landmarks, odometry edges: the optimised trajectory's map is
    closer to the true landmarks than the dead-reckoned one's, and its chi2 per
    degree of freedom is a usable consistency figure."""
    w = mr.world(seed)
    assert len(w["truth"]) == 72 and len(w["landmarks"]) == 16
    maps = [mr.landmark_map(w["halves"], 16, poses)
            for poses in (w["start"], mr.cpu_optimised(seed), w["truth"])]
    rms = [mr.map_rms(m[0], w["landmarks"]) for m in maps]
    dof = mr.chi2_per_dof(maps[1][2], maps[1][3])
    print("seed %d: %d half-edges, %d pair edges, map RMS start %.3f optimised %.3f truth %.3f, "
          "chi2/dof %.2f" % (seed, len(w["halves"]), len(w["edges"]), rms[0], rms[1], rms[2], dof))
    assert rms[1] < rms[0]
    assert dof < 2.0
    np.testing.assert_allclose(rms + [dof], TABLE[seed], rtol=0, atol=6e-3)
