"""EKF-SLAM update on the GPU at every operand width, tile edge and kernel path,
against the long-double restatement of tests/ekfslam_ref.py.

The bar, in every test: P entry by entry relative to max |P_prior|, mu
absolutely, each within max(1e-11, 64 x spread), where spread is the float64
oracle's own distance from the restatement (test_gpu_fastslam.py's rule and
floor; tests/test_ekfslam_ref.py shows the spread is below 1e-13 for every
case here, so the bar is 1e-11).  The device's P must also be exactly
symmetric, and every test asserts through DeviceEKFSLAM.info() that the
kernels it names are the ones that ran.  The update moves every 16 x 16 block
of P by at least 1e-6 of max |P_prior| (asserted on the CPU), so a skipped
tile, a stale operand quad or a wrong pad column stands five decades above
the bar.

Each test prints its worst device error next to the spread (pytest -s).
First green run on an MI355X: worst P error 3.48e-15 (repeated landmark,
k = 7; the float64 oracle's spread there is 3.48e-15), worst mu error 2.08e-15
(n = 384, k = 40; spread 1.93e-15); the multi-tile walk (n = 2820, 276 tiles on
a resident grid of 256) 1.75e-16 .. 9.6e-16 in P.  The device sits at the
float64 oracle's own rounding, four decades under the bar.
"""
import functools

import numpy as np
import pytest

import ekfslam_ref as er

pytestmark = pytest.mark.gpu

def _device(n_lm):
    from slamhip.ekf import DeviceEKFSLAM
    return DeviceEKFSLAM(n_lm, dt=er.DT, q_robot=er.Q_ROBOT, noise=er.NOISE)


def expected_path(k):
    """(M, rank-update kernel, apply kernel) of a default handle."""
    M = 4 * ((3 * k + 3) // 4)
    return (M, "frag2x4", "mfma") if k <= 21 else (M, "lds", "lds")


class Worst:
    """Collects (error / spread) pairs and prints the worst of a test."""

    def __init__(self, name):
        self.name, self.rows = name, []

    def add(self, tag, err, sp):
        self.rows.append((tag, err, sp))

    def report(self):
        if not self.rows:
            return
        wp = max(self.rows, key=lambda r: r[1][0])
        wm = max(self.rows, key=lambda r: r[1][1])
        print(f"\n{self.name}: worst P error {wp[1][0]:.3g} (spread {wp[2][0]:.3g}) at {wp[0]}; "
              f"worst mu error {wm[1][1]:.3g} (spread {wm[2][1]:.3g}) at {wm[0]}")


def check_state(case, mu_d, P_d, worst, tag):
    """The bar of this file for one device result."""
    assert np.array_equal(P_d, P_d.T), f"{tag}: P not symmetric"
    err, sp, bar = er.errors(case, mu_d, P_d), er.spread(case), er.bars(case)
    worst.add(tag, err, sp)
    if err[0] > bar[0]:
        D = np.abs((P_d - case.ld[1]).astype(np.float64)) / case.scale
        i, j = np.unravel_index(int(np.argmax(D)), D.shape)
        bad = np.argwhere(D > bar[0])
        raise AssertionError(
            f"{tag}: P error {err[0]:.3g} > {bar[0]:.3g} (spread {sp[0]:.3g}) at ({i}, {j}); "
            f"{len(bad)} entries over the bar, rows {bad[:, 0].min()}..{bad[:, 0].max()}, "
            f"columns {bad[:, 1].min()}..{bad[:, 1].max()}")
    assert err[1] <= bar[1], f"{tag}: mu error {err[1]:.3g} > {bar[1]:.3g} (spread {sp[1]:.3g})"


def check_info(info, case, M, rank, apply, tag):
    n = case.mu_p.size
    assert (info["n"], info["n_pad"]) == (n, (n + 127) // 128 * 128), (tag, info)
    assert info["ld"] == (n + 15) // 16 * 16 and info["ld"] >= n, (tag, info)
    nt = info["n_pad"] // 128
    assert info["n_tiles"] == nt * (nt + 1) // 2, (tag, info)
    assert (info["M"], info["rank"], info["apply"]) == (M, rank, apply), (tag, info)


def run_update(dev, case, path, worst, tag):
    """One update from the case's predicted state on handle ``dev``."""
    dev.set_state(case.mu_p, case.P_p)
    dev.update(case.ids, case.obs)
    mu_d, P_d = dev.get_state()
    check_info(dev.info(), case, *path, tag)
    check_state(case, mu_d, P_d, worst, tag)


def test_info_before_the_first_update():
    dev = _device(42)
    try:
        info = dev.info()
    finally:
        dev.close()
    assert (info["n"], info["ld"], info["n_pad"], info["n_tiles"]) == (129, 144, 256, 3)
    assert (info["M"], info["rank"], info["apply"]) == (0, None, None)
    assert info["frag_grid"] > 0 and info["frag_grid"] % 8 == 0
    assert info["pipe_grid"] > 0 and info["pipe_grid"] % 8 == 0


def test_all_widths_two_tile_rows():
    """k = 1 .. 40 at n = 129: one row past a tile, so 3 tiles and a last tile
    row with a single valid row.  Every M = 4 ceil(3k / 4) from 4 to 120, the
    m < M padding at every k not divisible by 4, every Q of the frag kernel,
    both sides of the M = 64 / 68 switch, LDS chunks of 4 .. 32."""
    worst = Worst("all widths, n = 129")
    dev = _device(42)
    try:
        assert dev.info()["ld"] == 144
        for n_lm, k in er.ALL_WIDTHS:
            path = expected_path(k)
            assert path[0] == 4 * -(-3 * k // 4)
            assert path[1:] == (("frag2x4", "mfma") if k <= 21 else ("lds", "lds"))
            run_update(dev, er.cached_case(n_lm, k), path, worst, f"k={k}")
    finally:
        dev.close()
        worst.report()


@pytest.mark.parametrize("n_lm", er.EDGE_SIZES)
def test_tile_and_line_edges(n_lm):
    """n = 6 and 15 (below 16), 18 (crosses 16), 48 (ld == n), 258 (two rows
    past two tiles), 384 (exactly three tiles), each with k in {1, 5, 21, 22,
    40} up to n_lm; ids unsorted and naming landmarks 0 and n_lm - 1."""
    worst = Worst(f"edges, n = {3 + 3 * n_lm}")
    dev = _device(n_lm)
    try:
        if n_lm == 15:
            assert dev.info()["ld"] == dev.info()["n"] == 48
        for nl, k in er.EDGES:
            if nl == n_lm:
                run_update(dev, er.cached_case(n_lm, k), expected_path(k), worst, f"k={k}")
    finally:
        dev.close()
        worst.report()


# ------------------------------------------------------ the multi-tile walk
def walk_size(grid, what):
    """n_lm at which a resident grid of ``grid`` workgroups has to walk: more
    tiles than workgroups, so some take two tiles and some one."""
    nt, n_lm = er.multi_tile_n_lm(grid)
    assert nt <= 40, f"{what} = {grid} would need nt = {nt} tile rows (n = {128 * (nt - 1) + 3})"
    return nt, n_lm


def check_walk(info, grid, nt):
    assert info["n_pad"] == 128 * nt and info["n_tiles"] == nt * (nt + 1) // 2, info
    per_xcd, stride = -(-info["n_tiles"] // 8), grid // 8
    # more tiles per XCD than workgroups per XCD, at most twice as many: some
    # workgroups walk two tiles, the rest (if any) one
    assert stride < per_xcd <= 2 * stride, (info, per_xcd, stride)


@functools.lru_cache(maxsize=1)
def big_case(n_lm, k):
    """A case too large for tests/test_ekfslam_ref.py's tables (its size comes
    from the device): the CPU conditions are asserted here."""
    case = er.world_case(n_lm, k)
    sp = er.spread(case)
    assert sp[0] <= 1e-13 and sp[1] <= 1e-13, sp
    assert er.min_block_change(case) >= 1e-6
    return er.slim(case)


@pytest.mark.parametrize("k", [1, 2, 3, 21])
def test_multi_tile_walk(k):
    """Q = 1, 2, 3 and 16 with more tiles than the resident grid holds: the
    ``more`` path of the frag kernel (pre -> acc carry-over, the next tile's
    first operand quads).  The whole matrix is compared."""
    worst = Worst(f"multi-tile walk, k = {k}")
    probe = _device(1)
    try:
        grid = probe.info()["frag_grid"]
    finally:
        probe.close()
    nt, n_lm = walk_size(grid, "frag_grid")
    dev = _device(n_lm)
    try:
        check_walk(dev.info(), grid, nt)
        run_update(dev, big_case(n_lm, k), expected_path(k), worst, f"n_lm={n_lm} nt={nt} k={k}")
    finally:
        dev.close()
        worst.report()


def test_variable_width_sequence_on_one_handle():
    """k = 40, 1, 21, 22, 3, 16 on one handle (predict + update each), the
    reference restarted from the device's own state before each step: stale
    columns of pht, kg, Kf, Hf, sinv or e after M shrinks would show."""
    worst = Worst("variable-width sequence, n = 384")
    _, _, mu, P = er.slam_world(er.SEQUENCE_N_LM, 77)
    dev = _device(er.SEQUENCE_N_LM)
    try:
        dev.set_state(mu, P)
        for step, k in enumerate(er.SEQUENCE):
            mu0, P0 = dev.get_state()
            ids, obs = er.sequence_observation(step, k)
            case = er.Case(mu0, P0, ids, obs)
            dev.step(er.CTL, ids, obs)
            mu_d, P_d = dev.get_state()
            check_info(dev.info(), case, *expected_path(k), f"step {step}")
            check_state(case, mu_d, P_d, worst, f"step {step} k={k}")
    finally:
        dev.close()
        worst.report()


@pytest.mark.parametrize("k", [2, 7])
def test_repeated_landmark(k):
    """One landmark named twice with two different measurements: H has two row
    blocks on the same columns."""
    worst = Worst(f"repeated landmark, k = {k}")
    case = er.cached_case(42, k, True)
    assert case.ids[0] == case.ids[-1] and not np.array_equal(case.obs[0], case.obs[-1])
    dev = _device(42)
    try:
        run_update(dev, case, expected_path(k), worst, f"ids={list(case.ids)}")
    finally:
        dev.close()
        worst.report()


def test_yaw_wraps_in_the_update():
    """Predicted yaw pi - 1e-3, observations taken from a pose whose yaw is
    pi + 0.05: mu + K e leaves (-pi, pi] and the update wraps it."""
    worst = Worst("yaw wrap")
    case = er.world_case(42, 8, yaw=np.pi - 1e-3, true_yaw=np.pi + 0.05)
    mu_l, _ = case.ld
    assert case.aux["yaw_unwrapped"] > np.pi + 1e-3          # from the restatement alone
    assert mu_l[2] == case.aux["yaw_unwrapped"] - 2 * er.LD(np.pi) and mu_l[2] < 0
    dev = _device(42)
    try:
        run_update(dev, case, expected_path(8), worst, "k=8")
        mu_d = dev.get_state(with_cov=False)
    finally:
        dev.close()
        worst.report()
    assert abs(mu_d[2] - float(mu_l[2])) <= er.bars(case)[1]
    assert -np.pi < mu_d[2] < -np.pi + 0.1


VARIANTS = [("SLAM_EKS_KERNEL", "pipe", 5, "pipe", "mfma"),
            ("SLAM_EKS_KERNEL", "pipe", 21, "pipe", "mfma"),
            ("SLAM_EKS_KERNEL", "frag16", 5, "frag2x2", "mfma"),
            ("SLAM_EKS_KERNEL", "frag16", 21, "frag2x2", "mfma"),
            ("SLAM_EKS_KERNEL", "pfmid", 20, "frag2x4_pf", "mfma"),
            ("SLAM_EKS_KERNEL", "pf0", 20, "frag2x4_pf", "mfma"),
            ("SLAM_EKS_APPLY", "lds", 5, "frag2x4", "lds")]


@pytest.mark.parametrize("var,value,k,rank,apply", VARIANTS)
def test_selected_variants(monkeypatch, var, value, k, rank, apply):
    """The environment-selected kernels (read when the handle is created) at
    n = 384, same bar."""
    worst = Worst(f"{var}={value}, k = {k}")
    monkeypatch.delenv("SLAM_EKS_KERNEL", raising=False)
    monkeypatch.delenv("SLAM_EKS_APPLY", raising=False)
    monkeypatch.setenv(var, value)
    dev = _device(127)
    try:
        run_update(dev, er.cached_case(127, k), (expected_path(k)[0], rank, apply), worst,
                   f"{var}={value} k={k}")
    finally:
        dev.close()
        worst.report()


@pytest.mark.parametrize("value,rank,grid_key", [("pipe", "pipe", "pipe_grid"),
                                                 ("frag16", "frag2x2", "frag_grid")])
def test_selected_variants_multi_tile(monkeypatch, value, rank, grid_key):
    """pipe and frag16 where their own resident grid has to walk, k = 2."""
    worst = Worst(f"SLAM_EKS_KERNEL={value}, multi-tile")
    monkeypatch.delenv("SLAM_EKS_APPLY", raising=False)
    monkeypatch.setenv("SLAM_EKS_KERNEL", value)
    probe = _device(1)
    try:
        grid = probe.info()[grid_key]
    finally:
        probe.close()
    nt, n_lm = walk_size(grid, grid_key)
    dev = _device(n_lm)
    try:
        check_walk(dev.info(), grid, nt)
        run_update(dev, big_case(n_lm, 2), (8, rank, "mfma"), worst, f"n_lm={n_lm} nt={nt} k=2")
    finally:
        dev.close()
        worst.report()


def test_bad_arguments_leave_the_state_alone():
    from slamhip._lib import SlamError
    case = er.cached_case(42, 5)
    good = case.obs[0]
    dev = _device(42)
    try:
        dev.set_state(case.mu_p, case.P_p)
        dev.update(case.ids, case.obs)
        mu0, P0 = dev.get_state()
        info0 = dev.info()
        for ids in ([], list(np.arange(41) % 42), [3, -1], [3, 42]):
            with pytest.raises(SlamError):
                dev.update(np.array(ids, dtype=np.int64), np.tile(good, (len(ids), 1)))
            mu1, P1 = dev.get_state()
            assert np.array_equal(mu0, mu1) and np.array_equal(P0, P1), ids
        assert dev.info() == info0
    finally:
        dev.close()


def test_get_rows_is_get_state():
    case = er.cached_case(127, 5)
    dev = _device(127)
    try:
        dev.set_state(case.mu_p, case.P_p)
        dev.update(case.ids, case.obs)
        _, P = dev.get_state()
        n = P.shape[0]
        rows = np.array([0, 2, 3, n - 1, 200, 200])
        assert np.array_equal(dev.get_rows(rows), P[rows])
        rows = np.random.RandomState(97).randint(0, n, 97)    # three batches of the id scratch
        assert np.array_equal(dev.get_rows(rows), P[rows])
        assert dev.get_rows(np.array([], dtype=np.int64)).shape == (0, n)
    finally:
        dev.close()
