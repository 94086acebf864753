"""The NumPy restatement of the robust edge weights (tests/graph_robust_ref.py,
DESIGN 8.3) against its own definitions, and the CPU table of the issue that
asked for them: one edge in ten of circle_graph(72, n_landmarks=16, seed) given
the obs_aft of another edge, Gauss-Newton with the reference's gate in place
until sum(delta^2) < 0.01 or 50 iterations, distance (RMS over the positions)
to the solution of the uncorrupted graph.

Seed 5 reproduces the issue's row.  The issue's row for seed 6 ("265 edges, 13
corrupted") is the run at one edge in TWENTY; its recipe (one in ten, 26
edges) gives the row asserted below.  Both are recorded in DESIGN 8.3.
"""
import numpy as np
import pytest

import graph_robust_ref as rr

K = [("huber", 1.0), ("huber", 2.0), ("cauchy", 2.0), ("dcs", 5.0)]


def test_weight_and_cost_at_zero_kink_and_far_out():
    for kind, k in K:
        w, rho = rr.weight_cost(np.array([0.0]), kind, k)
        assert w[0] == 1.0 and rho[0] == 0.0, kind
    w, rho = rr.weight_cost(np.array([0.0, 3.0, 1e9]), "none", 0.0)
    np.testing.assert_array_equal(w, 1.0)
    np.testing.assert_array_equal(rho, [0.0, 3.0, 1e9])
    # Huber's kink chi2 = k^2: w = 1 and rho = k^2 from both sides, continuous across it
    for k in (1.0, 2.0):
        k2 = k * k
        w, rho = rr.weight_cost(np.array([np.nextafter(k2, 0), k2, np.nextafter(k2, 9)]), "huber", k)
        assert w[0] == 1.0 and w[1] == 1.0 and abs(w[2] - 1.0) < 1e-15
        np.testing.assert_allclose(rho, k2, rtol=1e-15)
    # DCS's kink chi2 = Phi (s = 1)
    w, rho = rr.weight_cost(np.array([np.nextafter(5.0, 0), 5.0, np.nextafter(5.0, 9)]), "dcs", 5.0)
    np.testing.assert_allclose(w, 1.0, rtol=1e-15)
    np.testing.assert_allclose(rho, 5.0, rtol=1e-15)
    # far out: the closed forms
    c = 1e8
    w, rho = rr.weight_cost(np.array([c]), "huber", 2.0)
    np.testing.assert_allclose([w[0], rho[0]], [2.0 / 1e4, 2 * 2.0 * 1e4 - 4.0], rtol=1e-15)
    w, rho = rr.weight_cost(np.array([c]), "cauchy", 2.0)
    np.testing.assert_allclose([w[0], rho[0]], [1.0 / (1 + c / 4), 4 * np.log(1 + c / 4)], rtol=1e-15)
    w, rho = rr.weight_cost(np.array([c]), "dcs", 5.0)
    s = 10.0 / (5.0 + c)
    np.testing.assert_allclose([w[0], rho[0]], [s * s, s * s * c + 5.0 * (1 - s) ** 2], rtol=1e-15)
    # every weight lies in (0, 1] and falls with chi2
    x = np.linspace(0.0, 50.0, 2001)
    for kind, k in K:
        w, _ = rr.weight_cost(x, kind, k)
        assert np.all(w > 0) and np.all(w <= 1) and np.all(np.diff(w) <= 0), kind


@pytest.mark.parametrize("kind,k", [("huber", 1.0), ("huber", 2.0), ("cauchy", 2.0)])
def test_weight_is_the_derivative_of_the_cost(kind, k):
    """rho'(chi2) = w by central differences (away from Huber's kink, where rho'
    has its corner: the step stays on one side)."""
    x = np.concatenate([np.linspace(0.05, k * k - 0.05, 40), np.linspace(k * k + 0.05, 400.0, 400)])
    h = 1e-5
    d = (rr.weight_cost(x + h, kind, k)[1] - rr.weight_cost(x - h, kind, k)[1]) / (2 * h)
    w = rr.weight_cost(x, kind, k)[0]
    # truncation h^2 |rho'''| / 6 <= 1e-10 / 6 * 0.7; rounding of the difference
    # 2 * 1.1e-16 * rho / (2 h) <= 1.1e-16 * 80 / 1e-5 = 9e-10
    np.testing.assert_allclose(d, w, rtol=0, atol=5e-9)


def test_chi2_is_the_edge_cost_of_the_oracle():
    """The restatement against graph_oracle: with w = 1 the scaled update is the
    oracle's update bit for bit, and chi2_e = err^T Omega err agrees with the
    oracle's own right-hand side b_A = Ja^T Omega err (Ja is invertible: chi2 =
    err . Ja^-T b_A)."""
    import graph_oracle as go
    init, _, rec, cor, _ = rr.corrupted_graph(5)
    edges = rr.edge_rows(cor)[:40]
    a = rr.update_est_pose(edges, init, None, None)
    b = go.update_est_pose(edges, init)
    for u, v in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(u, v)
    chi2, w, rho = rr.chi2_weights(edges, init, "none", 0.0)
    assert np.all(chi2 >= 0) and np.all(w == 1) and np.array_equal(rho, chi2)
    # b_A = Ja^T Omega err: chi2 = err^T (Ja^-T b_A)
    blocks = go.linearize(edges, init)
    for e, blk, c in zip(edges, blocks, chi2):
        err, info = rr.edge_err_info(e, init)
        xa = init[int(e[6])]
        th = go.wrap_angle(xa[2] + e[8])
        ja = np.array([[1, 0, -e[7] * np.sin(th)], [0, 1, e[7] * np.cos(th)], [0, 0, 1]])
        np.testing.assert_allclose(err @ np.linalg.solve(ja.T, blk[39:42]), c, rtol=1e-9, atol=1e-12)


# distance to the clean solution (m): plain, huber 1.0, huber 2.0, cauchy 2.0, dcs 5.0
TABLE = {5: (264, 26, [3.02, 0.39, 0.41, 0.29, 0.30]),
         6: (265, 26, [1.92, 0.31, 0.35, 0.34, 0.37])}
# edges with w < 0.1 under cauchy 2.0 and dcs 5.0: (corrupted, clean)
LOW = {5: (26, 5), 6: (26, 3)}


@pytest.mark.parametrize("seed", [5, 6])
def test_cpu_table(seed):
    E, n_bad, row = TABLE[seed]
    init, truth, rec, cor, mask = rr.corrupted_graph(seed)
    assert len(rec) == E and mask.sum() == n_bad
    clean, st0, _, _ = rr.cpu_run(seed, None, None, corrupted=False)
    assert np.all(st0[:, 0] == 1.0)
    got = []
    for kind, k in [(None, None)] + K:
        p, st, chi2, w = rr.cpu_run(seed, kind, k)
        assert np.all(st[:, 0] == 1.0), (seed, kind, k)       # the gate passes every iteration
        assert len(st) < 50 and st[-1, 1] < 0.01
        got.append(rr.position_rms(p, clean))
        if (kind, k) in (("cauchy", 2.0), ("dcs", 5.0)):
            low = w < 0.1
            assert ((low & mask).sum(), (low & ~mask).sum()) == LOW[seed], (seed, kind)
    print("seed", seed, "distances", got)
    np.testing.assert_allclose(got, row, rtol=0, atol=0.005)  # the table's two decimals
    assert min(got[0] / g for g in got[1:]) > (7.0 if seed == 5 else 5.0)


def test_issue_row_of_seed_6_is_one_edge_in_twenty():
    """The issue's seed-6 row (1.33 m plain, 0.27 under cauchy 2.0, 13 of 13
    corrupted edges and 3 clean ones below w = 0.1)."""
    init, truth, rec, cor, mask = rr.corrupted_graph(6, frac=0.05)
    assert mask.sum() == 13
    clean = rr.cpu_run(6, None, None, corrupted=False)[0]
    edges = rr.edge_rows(cor)
    plain, st = rr.gauss_newton(edges, init)
    assert np.all(st[:, 0] == 1.0)
    p, st = rr.gauss_newton(edges, init, "cauchy", 2.0)
    assert np.all(st[:, 0] == 1.0)
    w = rr.chi2_weights(edges, p, "cauchy", 2.0)[1]
    np.testing.assert_allclose([rr.position_rms(plain, clean), rr.position_rms(p, clean)],
                               [1.33, 0.27], rtol=0, atol=0.005)
    assert ((w < 0.1) & mask).sum() == 13 and ((w < 0.1) & ~mask).sum() == 3
