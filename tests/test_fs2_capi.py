"""FastSLAM 2.0 proposal handles, C-ABI, CPU side: slam_fs_create_proposal's
argument checks return SLAM_ERR_ARG before any HIP call (no device needed),
slam_fs_get_proposal refuses a NULL handle, and the ctypes struct matches the
header."""
import ctypes as C

import pytest

from conftest import PKG  # noqa: F401  (puts the package on sys.path)


@pytest.fixture(scope="module")
def lib():
    from slamhip import _lib
    return _lib.load()


def _cfg(motion="linear", **kw):
    from slamhip._lib import FSConfig
    from slamhip.pf import make_config
    c = FSConfig()
    c.pf = make_config(100, motion=motion)
    c.r_dist, c.r_dir, c.r_orient, c.use_orient = 0.1, 0.05, 0.05, 1
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _pcfg(record=1):
    from slamhip._lib import FSProposalConfig
    return FSProposalConfig(int(record), 0)


def test_create_proposal_argument_errors_without_a_device(lib):
    from slamhip._lib import SLAM_ERR_ARG

    def create(c, a, n, nl, out=True):
        h = C.c_void_p()
        rc = lib.slam_fs_create_proposal(None if c is None else C.byref(c),
                                         None if a is None else C.byref(a), n, nl, 0,
                                         C.byref(h) if out else None)
        assert not h.value
        return rc, lib.slam_last_error().decode()

    rc, msg = create(None, _pcfg(), 100, 8)
    assert rc == SLAM_ERR_ARG and "cfg" in msg
    rc, msg = create(_cfg(), None, 100, 8)
    assert rc == SLAM_ERR_ARG and "pcfg" in msg
    rc, msg = create(_cfg(), _pcfg(), 100, 8, out=False)
    assert rc == SLAM_ERR_ARG and "out" in msg
    rc, msg = create(_cfg(motion="velocity"), _pcfg(), 100, 8)
    assert rc == SLAM_ERR_ARG and "motion" in msg, (rc, msg)
    # slam_fs_create's rules
    for n in (0, -1, (1 << 24) + 1):
        rc, msg = create(_cfg(), _pcfg(), n, 8)
        assert rc == SLAM_ERR_ARG and "n_particles" in msg, (n, rc, msg)
    for nl in (0, -3):
        rc, msg = create(_cfg(), _pcfg(), 100, nl)
        assert rc == SLAM_ERR_ARG and "n_landmarks" in msg, (nl, rc, msg)
    rc, msg = create(_cfg(r_dist=0.0), _pcfg(), 100, 8)
    assert rc == SLAM_ERR_ARG and "r_dist" in msg


def test_get_proposal_refuses_a_null_handle(lib):
    from slamhip._lib import SLAM_ERR_ARG
    d = (C.c_double * 6)()
    assert lib.slam_fs_get_proposal(None, d, d, d) == SLAM_ERR_ARG
    assert b"slam_fs_get_proposal" in lib.slam_last_error()
    assert lib.slam_fs_get_proposal(None, None, None, None) == SLAM_ERR_ARG


def test_config_struct_matches_the_header():
    from slamhip import _lib
    assert C.sizeof(_lib.FSProposalConfig) == 8
    assert _lib.FSProposalConfig.record.offset == 0 and _lib.FSProposalConfig.pad0.offset == 4
    assert _lib.FS_PROPOSAL == ("motion", "measurement")
    for name in ("slam_fs_create_proposal", "slam_fs_get_proposal"):
        assert name in _lib.SIGNATURES


def test_front_end_argument_errors():
    from slamhip.fastslam import DeviceFastSLAM
    with pytest.raises(ValueError, match="proposal"):
        DeviceFastSLAM(10, 3, proposal="optimal")
    with pytest.raises(ValueError, match="association"):
        DeviceFastSLAM(10, 3, proposal="measurement", association="ml")
