"""The NumPy restatement of the odometry edges (tests/graph_odom_ref.py, DESIGN
8.4) against its own definitions, and the CPU table of DESIGN 8.4:
circle_graph(72, n_landmarks=16, seed) clean and with one pairing in ten wrong (graph_robust_ref.corrupted_graph), with and without one odometry edge
per consecutive pose pair (sigma 0.02, 0.02, 0.01), plain and under cauchy 2.0;
Gauss-Newton with the reference's gate in place until sum(delta^2) < 0.01 or 50
iterations; RMS position distance to TRUTH and the iteration count.

The table was first run as a throw-away experiment; the restatement reproduces
it to three decimals (one cell, seed 5, corrupted, plain + odometry, is 1.15945
here and was noted as "1.160": a rounding of the same number).
"""
import numpy as np
import pytest

import graph_odom_ref as gr
import graph_robust_ref as rr


def test_jacobians_agree_with_central_differences():
    """J_b and J_a against central differences of err (step 1e-6) at random
    poses, theta differences across +-pi included.  Truncation: h^2 |err'''| / 6
    <= 1e-12 * 30 / 6; rounding of the difference: 2 * 1.1e-16 * 30 / 2e-6 =
    3.3e-9 at |err| <= 30 -- the bar is 1e-8."""
    rs = np.random.RandomState(3)
    h = 1e-6
    worst = 0.0
    for trial in range(200):
        poses = np.column_stack([rs.uniform(-10, 10, (2, 2)), rs.uniform(-np.pi, np.pi, 2)])
        if trial % 4 == 0:                                  # theta_a - theta_b across +-pi
            poses[0, 2] = np.pi - 0.01 * rs.rand()
            poses[1, 2] = -np.pi + 0.01 * rs.rand()
        if trial % 4 == 1:
            poses[0, 2] = -np.pi + 0.01 * rs.rand()
            poses[1, 2] = np.pi - 0.01 * rs.rand()
        z = gr.relpose(poses[0], poses[1]) + rs.normal(0, 0.05, 3)
        row = [0, 0, 1, 1, *z, 0.02, 0.02, 0.01]
        err, info, jb, ja = gr.odom_err_info(row, poses)
        assert np.all(np.abs(err) < 1.0)                    # wrapped: no 2 pi jump in the residual
        np.testing.assert_array_equal(info, np.diag([2500.0, 2500.0, 10000.0]))
        for which, jac in ((0, jb), (1, ja)):
            num = np.empty((3, 3))
            for k in range(3):
                p, m = poses.copy(), poses.copy()
                p[which, k] += h
                m[which, k] -= h
                d = gr.odom_err_info(row, p)[0] - gr.odom_err_info(row, m)[0]
                d[2] = gr.wrap_angle(d[2])
                num[:, k] = d / (2 * h)
            worst = max(worst, np.abs(num - jac).max())
    print("max |J - central difference|", worst)
    assert worst < 1e-8


def test_relpose_is_invariant_under_a_rigid_motion():
    from slamhip.graph import relpose
    rs = np.random.RandomState(4)
    for _ in range(100):
        xb = np.array([*rs.uniform(-10, 10, 2), rs.uniform(-np.pi, np.pi)])
        xa = np.array([*rs.uniform(-10, 10, 2), rs.uniform(-np.pi, np.pi)])
        rel = relpose(xb, xa)
        # the package's is the restatement's; the two wrap in different forms, each
        # with roundings at magnitude <= 2 pi (ulp 8.9e-16)
        np.testing.assert_allclose(rel, gr.relpose(xb, xa), rtol=0, atol=2e-15)
        phi, t = rs.uniform(-np.pi, np.pi), rs.uniform(-20, 20, 2)
        R = np.array([[np.cos(phi), -np.sin(phi)], [np.sin(phi), np.cos(phi)]])
        mb = np.array([*(R @ xb[:2] + t), xb[2] + phi])
        ma = np.array([*(R @ xa[:2] + t), xa[2] + phi])
        moved = relpose(mb, ma)
        # |coordinates| <= 50: 1e-13 is ~15 roundings of that size
        np.testing.assert_allclose(moved[:2], rel[:2], rtol=0, atol=1e-13)
        assert abs(gr.wrap_angle(moved[2] - rel[2])) < 1e-13
    # the rel of a commanded step does not depend on where it starts: robot +y
    # forward and BASE_ANG do not enter
    step = relpose([0.0, 0.0, 0.0], [1.0, 2.0, 0.3])
    np.testing.assert_allclose(relpose([3.0, -4.0, 0.0], [4.0, -2.0, 0.3]), step, rtol=0, atol=1e-15)


def test_odometry_only_chain_reproduces_rel():
    """n_edges = 0: the chain has a zero-residual solution, Gauss-Newton reaches
    it (chi2 <= 1e-20), consecutive poses reproduce rel and pose 0 stays where
    the anchor left it."""
    T = 40
    rs = np.random.RandomState(11)
    rel = np.column_stack([rs.uniform(0.5, 1.5, T - 1), rs.uniform(-0.2, 0.2, T - 1),
                           rs.uniform(-0.3, 0.3, T - 1)])
    odom = np.array([[k, k, k + 1, k + 1, *rel[k], 0.02, 0.02, 0.01] for k in range(T - 1)])
    init = np.column_stack([np.cumsum(rs.normal(1.0, 0.3, T)), rs.normal(0, 0.5, T),
                            rs.uniform(-0.5, 0.5, T)])
    poses, st = gr.gauss_newton(np.empty((0, 11)), odom, init, max_iter=50, delta_sum_th=1e-24)
    assert np.all(st[:, 0] == 1.0) and len(st) < 50
    chi2 = gr.chi2_weights(np.empty((0, 11)), odom, poses)[0]
    print("iterations", len(st), "sum chi2", chi2.sum())
    assert chi2.sum() <= 1e-20
    for k in range(T - 1):
        got = gr.relpose(poses[k], poses[k + 1])
        np.testing.assert_allclose(got, rel[k], rtol=0, atol=1e-12)
    # the closed form: the rels composed from pose 0, wherever the anchored solves left it
    closed = np.empty((T, 3))
    closed[0] = poses[0]
    for k in range(T - 1):
        c, s = np.cos(closed[k, 2]), np.sin(closed[k, 2])
        closed[k + 1] = [closed[k, 0] + c * rel[k, 0] - s * rel[k, 1],
                         closed[k, 1] + s * rel[k, 0] + c * rel[k, 1],
                         gr.wrap_angle(closed[k, 2] + rel[k, 2])]
    np.testing.assert_allclose(poses, closed, rtol=0, atol=1e-10)


# (RMS to truth in metres, iterations): plain without / with odometry, cauchy 2.0
# without / with odometry -- the restatement's values, to three decimals
# (see the module docstring for the 1.159 cell)
TABLE = {
    (5, False): [(0.890, 36), (0.243, 5), (0.804, 14), (0.304, 9)],
    (5, True): [(3.083, 47), (1.159, 10), (0.818, 14), (0.338, 8)],
    (6, False): [(0.625, 30), (0.512, 3), (0.607, 14), (0.473, 4)],
    (6, True): [(1.827, 28), (1.520, 11), (0.569, 14), (0.406, 3)],
}


@pytest.mark.parametrize("seed,corrupted", sorted(TABLE))
def test_cpu_table(seed, corrupted):
    truth = rr.corrupted_graph(seed)[1]
    got = []
    for kind, k in ((None, None), ("cauchy", 2.0)):
        cell = []
        for with_odom in (False, True):
            p, st = gr.cpu_run(seed, kind, k, corrupted, with_odom)
            assert np.all(st[:, 0] == 1.0), (seed, corrupted, kind, with_odom)   # is_calc = 1 throughout
            cell.append((rr.position_rms(p, truth), len(st)))
        # odometry: nearer to truth, and in no more iterations
        assert cell[1][0] < cell[0][0] and cell[1][1] <= cell[0][1], (seed, corrupted, kind, cell)
        got += cell
    print("seed", seed, "corrupted", corrupted, got)
    for (d, n), (d_ref, n_ref) in zip(got, TABLE[(seed, corrupted)]):
        assert n == n_ref and abs(d - d_ref) <= 0.00051, (got, TABLE[(seed, corrupted)])


def test_without_odometry_the_mixed_restatement_is_the_robust_one():
    init, _, _, cor, _ = rr.corrupted_graph(5)
    edges = rr.edge_rows(cor)[:60]
    a = gr.update_est_pose(edges, np.empty((0, 10)), init, "cauchy", 2.0)
    b = rr.update_est_pose(edges, init, "cauchy", 2.0)
    for u, v in zip(a[:7], b):
        np.testing.assert_array_equal(u, v)
    # odometry weights are 1 under every kind, the landmark ones are not touched
    odom = gr.odom_rows(gr.odometry(5))
    for kind, k in rr.CASES:
        c, w, rho = gr.chi2_weights(edges, odom, init, kind, k)
        assert np.all(w[60:] == 1.0) and np.array_equal(rho[60:], c[60:])
        c0, w0, rho0 = rr.chi2_weights(edges, init, kind, k)
        np.testing.assert_array_equal(w[:60], w0)
