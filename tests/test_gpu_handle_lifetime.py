"""Every handle gives back exactly what it took.

The library's one allocator (csrc/device_mem.hpp) counts the device bytes,
pinned host bytes and events it holds in this process
(slam_debug_live_resources).  Each case reads the three counts, creates a
handle, checks that the device bytes rose (so the case cannot pass on a counter
that never moves), drives the handle through its regrow paths, destroys it and
requires all three counts to equal the first reading exactly.  The counts are
the library's own, so other users of the card do not move them.

The stateless entry points' scratch is process-lifetime by design: that case
asserts how it grows, not a return to the first reading.
"""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CTL = (1.0, 0.1)


def live():
    from slamhip import _lib
    out = (C.c_int64 * 3)()
    _lib.check(_lib.load().slam_debug_live_resources(out), "slam_debug_live_resources")
    return tuple(out)


class Balanced:
    """with Balanced() as b: ... b.created() after the create ... destroy."""

    def __enter__(self):
        gc.collect()                      # handles earlier tests left to the collector
        self.first = live()
        return self

    def created(self):
        now = live()
        assert now[0] > self.first[0], (self.first, now)
        return now

    def __exit__(self, et, ev, tb):
        if et is None:
            assert live() == self.first


def _landmarks(nl):
    return np.random.RandomState(5).uniform(-10.0, 10.0, (nl, 2))


def _z(lm, steps=None):
    import pf_oracle as po
    z = po.to_robot_frame(np.array([10.0, 0.0, np.pi / 2]), lm)
    return z if steps is None else np.tile(z, (steps, 1, 1))


def test_pf_regrows_and_rng_stream():
    from slamhip import _lib
    from slamhip.pf import DeviceParticleFilter
    lm = _landmarks(3)
    with Balanced() as b:
        pf = DeviceParticleFilter(1000, lm, motion="velocity", likelihood="logsum", seed=3)
        c0 = b.created()
        pf.load_observations(_z(lm, 1))
        assert live() == c0                                   # one step fits the create's arrays
        pf.load_observations(_z(lm, 9))                       # ensure_steps regrows
        c1 = live()
        assert c1[0] > c0[0] and c1[1] > c0[1], (c0, c1)
        assert len(pf.run(0, np.tile(CTL, (9, 1)))) == 9
        assert live() == c1
        pf.enable_timing(True)                                # the timer's events
        pf.step(CTL, _z(lm))
        assert live()[2] > c1[2]
        pf.enable_timing(False)
        c2 = live()
        pf.use_numpy_stream(np.random.RandomState(7).get_state())      # mt_reserve allocates
        for _ in range(2):
            pf.step_truth(CTL, np.array([10.0, 0.0, np.pi / 2]))
        assert live()[0] > c2[0]
        lib = _lib.load()
        _lib.check(lib.slam_pf_set_stream(pf._h, None, 1), "slam_pf_set_stream")   # the default stream
        _lib.check(lib.slam_pf_set_stream(pf._h, None, 0), "slam_pf_set_stream")   # an owned one again
        pf.close()


def test_pf_slice_prepass_buffers():
    from slamhip.pf import DeviceParticleFilter
    with Balanced() as b:
        pf = DeviceParticleFilter((1 << 20) + 4096, _landmarks(3))
        b.created()
        pf.close()


def test_pfb_result_and_control_buffers_grow():
    from slamhip.pf_batch import BatchParticleFilter
    lm = _landmarks(3)
    B = 3
    with Balanced() as b:
        e = BatchParticleFilter(B, 100, lm)
        c0 = b.created()
        e.step(CTL, np.tile(_z(lm), (B, 1, 1)))
        assert live() == c0
        e.load_observations(np.tile(_z(lm), (5, B, 1, 1)))
        e.run(0, np.tile(CTL, (5, 1)))
        c1 = live()
        assert c1[0] > c0[0] and c1[1] > c0[1], (c0, c1)
        e.close()


OBS = np.array([[5.0, 0.1, 0.2], [6.0, -0.3, 0.1], [7.0, 0.4, -0.2]])


def test_fs_obs_and_stage_buffers_grow():
    from slamhip.fastslam import DeviceFastSLAM
    with Balanced() as b:
        fs = DeviceFastSLAM(256, 4)
        c0 = b.created()
        fs.step(CTL, np.array([0]), OBS[:1])
        c1 = live()
        assert c1[0] > c0[0]                                  # fs_reserve_obs: 1 observation
        fs.step(CTL, np.array([0, 1, 2]), OBS)
        c2 = live()
        assert c2[0] > c1[0]                                  # ... regrown for 3
        fs.get_maps()
        assert live()[0] > c2[0]                              # fs_reserve_stage
        fs.close()


def test_fs_assoc_record_buffer_grows():
    from slamhip.fastslam import DeviceFastSLAM
    with Balanced() as b:
        fs = DeviceFastSLAM(256, 4, association="ml", record_assoc=True)
        c0 = b.created()
        assert c0[1] > b.first[1]                             # the pinned count word
        fs.update(None, OBS[:1])
        c1 = live()
        fs.update(None, OBS)                                  # fs_reserve_assoc (and obs) regrow
        assert live()[0] > c1[0] > c0[0]
        fs.close()


def test_ekf_staging_grows():
    from slamhip.ekf import DeviceEKF
    with Balanced() as b:
        ekf = DeviceEKF(4)
        c0 = b.created()
        z = np.tile([10.0, 0.0], (6, 4, 1))
        ekf.run(z[:1])
        c1 = live()
        ekf.run(z)
        assert live()[0] > c1[0] > c0[0]
        ekf.close()


def test_ekfslam_smallest_width():
    import ekfslam_ref as er
    from slamhip.ekf import DeviceEKFSLAM
    case = er.cached_case(1, 1)
    with Balanced() as b:
        dev = DeviceEKFSLAM(1, dt=er.DT, q_robot=er.Q_ROBOT, noise=er.NOISE)
        c0 = b.created()
        assert c0[2] > b.first[2]                             # its timing events
        dev.set_state(case.mu_p, case.P_p)
        dev.predict(CTL)
        dev.update(case.ids, case.obs)
        assert live() == c0
        dev.close()


def test_graph_poses_arena_and_dense_list():
    import graph_oracle as go
    from conftest import golden
    from slamhip.graph import DeviceGraph
    g = golden("graph")
    with Balanced() as b:
        dev = DeviceGraph(solver="dense")
        c0 = live()
        assert c0[1] > b.first[1] and c0[2] > b.first[2]      # pinned states, events: no device memory yet
        for i in (0, 3, 0):                                   # 2 poses, 3 poses, 2 again
            dev.set_poses(g[f"demo{i}_poses_before"])
            dev.set_edges(go.edges_from_pairs(g[f"demo{i}_pairs"]))
            dev.update()
        b.created()
        dev.close()


def test_dist_local_two_shards():
    from slamhip.dist import DistFilter
    lm = _landmarks(5)
    with Balanced() as b:
        d = DistFilter(2 * 8192 + 1000, lm, world=2, motion="velocity", likelihood="product", seed=9)
        b.created()
        d.step(CTL, _z(lm))
        d.close()


def test_mt_standalone():
    from slamhip.rng import DeviceRandomState
    with Balanced() as b:
        rs = DeviceRandomState(np.random.RandomState(11).get_state())
        b.created()
        assert rs.standard_normal(1000).shape == (1000,)
        rs.close()


def _grows(call, nbytes):
    """call(n) uses a per-device scratch of nbytes(n): find a size at which it
    grows (earlier tests of this process may have grown it already), then every
    further growth raises the device bytes by exactly the difference, and a
    repeat at the same size by nothing."""
    n, before = 1000, live()
    call(n)
    while live() == before:
        n *= 2
        assert n <= 1 << 22, "the scratch never grew"
        call(n)
    c1 = live()
    call(n)
    assert live() == c1
    call(2 * n)
    c2 = live()
    assert c2 == (c1[0] + nbytes(2 * n) - nbytes(n), c1[1], c1[2])
    call(2 * n)
    call(n)                                                   # smaller: the buffer stays
    assert live() == c2


def test_static_scratch_grows_once_per_size():
    from slamhip import _lib
    from slamhip._lib import check, dptr
    lib = _lib.load()
    lm = _landmarks(4)

    def al256(x):
        return (x + 255) // 256 * 256

    def detect(n):
        poses, cs = np.zeros((n, 3)), np.tile([1.0, 0.0, 0.0], (n, 1))
        det, obs = np.empty((n, 4), dtype=np.int32), np.empty((n, 4, 3))
        check(lib.slam_scan_detect(n, dptr(poses), dptr(cs), 4, dptr(lm), 5.0, 1.0,
                                   det.ctypes.data_as(_lib._I32), dptr(obs), 0), "slam_scan_detect")

    def ellipse(n):
        covs, out = np.tile([2.0, 0.5, 0.5, 1.0], (n, 1)), np.empty((n, 3))
        check(lib.slam_error_ellipse(n, dptr(covs), 3.0, 0, dptr(out), 0), "slam_error_ellipse")

    def motion(n):
        params, poses, out = np.array([0.1] * 7), np.zeros((n, 3)), np.empty((n, 3))
        check(lib.slam_motion_velocity(dptr(params), n, dptr(poses), 1.0, 0.1, None, dptr(out), 0),
              "slam_motion_velocity")

    _grows(detect, lambda n: 2 * al256(24 * n) + al256(16 * 4) + al256(4 * 4 * n) + al256(24 * 4 * n))
    _grows(ellipse, lambda n: 56 * n)
    _grows(motion, lambda n: 72 * n)
