"""EKF-SLAM long-double restatement (tests/ekfslam_ref.py), CPU side: for
every case table of tests/test_gpu_ekfslam_widths.py

* the float64 oracle's ekfslam_step lies within 1e-13 of the restatement
  (P relative to max |P_prior|, mu absolute) -- so the device bar
  max(1e-11, 64 x spread) is its floor of 1e-11 everywhere;
* the oracle's row form ekfslam_update_rows agrees on sampled rows to the same
  figure;
* the update moves every 16 x 16 block of P's lower triangle by at least 1e-6
  of max |P_prior|: a skipped or stale block stands five decades above the bar.

(The multi-tile cases of the GPU file depend on the device's resident grid;
that test asserts the same three conditions itself.)
"""
import numpy as np
import pytest

from conftest import ORACLE  # noqa: F401  (puts the oracle on sys.path)

import ekf_oracle as eo
import ekfslam_ref as er

SPREAD_MAX = 1e-13
BLOCK_MIN = 1e-6


def check_case(case, seed=0):
    sp_P, sp_mu = er.spread(case)
    assert sp_P <= SPREAD_MAX and sp_mu <= SPREAD_MAX, (sp_P, sp_mu)
    n = case.mu_p.size
    rs = np.random.RandomState(seed)
    rows = np.unique(np.concatenate([[0, 2, n - 1], rs.randint(0, n, 8)]))
    idx = [0, 1, 2]
    for j in case.ids:
        idx += [3 + 3 * j, 4 + 3 * j, 5 + 3 * j]
    mu_r, P_r = eo.ekfslam_update_rows(case.mu_p, case.P_p[idx], case.P_p[rows], rows, case.ids,
                                       case.obs, er.NOISE)
    mu_l, P_l = case.ld
    assert np.abs(mu_r - mu_l).max() <= SPREAD_MAX
    assert np.abs(P_r - P_l[rows]).max() <= SPREAD_MAX * case.scale
    assert er.min_block_change(case) >= BLOCK_MIN
    assert er.bars(case) == (1e-11, 1e-11)
    return sp_P, sp_mu


def test_gauss_jordan_inverse_in_long_double():
    rs = np.random.RandomState(3)
    for m in (1, 3, 24, 120):
        a = rs.normal(0, 1, (m, m))
        S = (a @ a.T + m * np.eye(m)).astype(er.LD)
        # a leading zero forces a row exchange
        if m > 1:
            S[0, 0] = 0
        Si = er.inv_gauss_jordan(S)
        assert Si.dtype == er.LD
        assert np.abs(S @ Si - np.eye(m)).max() <= 1e-15
        assert np.abs(Si.astype(np.float64) - np.linalg.inv(S.astype(np.float64))).max() <= 1e-12


def test_restatement_keeps_long_double_and_symmetry():
    case = er.cached_case(5, 5)
    mu_l, P_l = case.ld
    assert mu_l.dtype == er.LD and P_l.dtype == er.LD
    assert np.array_equal(P_l, P_l.T)
    # long double carries more than float64 here (x87 extended or wider)
    assert np.finfo(er.LD).eps < 1e-18


@pytest.mark.parametrize("n_lm,k", er.ALL_WIDTHS)
def test_all_widths_cases(n_lm, k):
    check_case(er.cached_case(n_lm, k))


@pytest.mark.parametrize("n_lm,k", er.EDGES)
def test_edge_cases(n_lm, k):
    case = er.cached_case(n_lm, k)
    if k >= 2:
        assert 0 in case.ids and n_lm - 1 in case.ids
        assert list(case.ids) != sorted(case.ids)
    check_case(case)


def test_repeated_landmark_cases():
    for k in (2, 7):
        case = er.cached_case(42, k, True)
        assert len(set(case.ids)) == k - 1
        check_case(case)


def test_variable_width_sequence_cases():
    """The sequence on the float64 oracle's own chain of states (on the device
    each step starts from the device's state)."""
    _, _, mu, P = er.slam_world(er.SEQUENCE_N_LM, 77)
    for step, k in enumerate(er.SEQUENCE):
        ids, obs = er.sequence_observation(step, k)
        case = er.Case(mu, P, ids, obs)
        check_case(case, step)
        mu, P = case.f64


def test_yaw_wrap_case_crosses_pi():
    case = er.world_case(42, 8, yaw=np.pi - 1e-3, true_yaw=np.pi + 0.05)
    assert abs(case.mu_p[2] - (np.pi - 1e-3)) < 1e-12
    mu_l, _ = case.ld
    assert case.aux["yaw_unwrapped"] > np.pi + 1e-3
    assert mu_l[2] < -np.pi + 0.1
    check_case(case)
