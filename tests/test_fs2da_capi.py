"""FastSLAM 2.0 without ids, C-ABI and front end, CPU side:
slam_fs_create_assoc_proposal's argument checks return SLAM_ERR_ARG before any
HIP call (no device needed) and name the offending argument, the binding knows
the symbol, and association="ml_marginal" asks for proposal="measurement"."""
import ctypes as C

import numpy as np
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


def _acfg(log_p_new=np.log(0.1), record=1):
    from slamhip._lib import FSAssocConfig
    return FSAssocConfig(float(log_p_new), int(record), 0)


def _pcfg(record=1):
    from slamhip._lib import FSProposalConfig
    return FSProposalConfig(int(record), 0)


def test_create_assoc_proposal_argument_errors_without_a_device(lib):
    from slamhip._lib import SLAM_ERR_ARG

    def create(c, a, p, n, cap, out=True):
        h = C.c_void_p()
        rc = lib.slam_fs_create_assoc_proposal(None if c is None else C.byref(c),
                                               None if a is None else C.byref(a),
                                               None if p is None else C.byref(p), n, cap, 0,
                                               C.byref(h) if out else None)
        assert not h.value
        return rc, lib.slam_last_error().decode()

    rc, msg = create(None, _acfg(), _pcfg(), 100, 8)
    assert rc == SLAM_ERR_ARG and "NULL cfg" in msg, (rc, msg)
    rc, msg = create(_cfg(), None, _pcfg(), 100, 8)
    assert rc == SLAM_ERR_ARG and "acfg" in msg, (rc, msg)
    rc, msg = create(_cfg(), _acfg(), None, 100, 8)
    assert rc == SLAM_ERR_ARG and "pcfg" in msg, (rc, msg)
    rc, msg = create(_cfg(), _acfg(), _pcfg(), 100, 8, out=False)
    assert rc == SLAM_ERR_ARG and "out" in msg, (rc, msg)
    for bad in (np.inf, -np.inf, np.nan):
        rc, msg = create(_cfg(), _acfg(log_p_new=bad), _pcfg(), 100, 8)
        assert rc == SLAM_ERR_ARG and "log_p_new" in msg, (bad, rc, msg)
    for cap in (0, -3):
        rc, msg = create(_cfg(), _acfg(), _pcfg(), 100, cap)
        assert rc == SLAM_ERR_ARG and "max_landmarks" in msg, (cap, rc, msg)
    rc, msg = create(_cfg(motion="velocity"), _acfg(), _pcfg(), 100, 8)
    assert rc == SLAM_ERR_ARG and "motion" in msg, (rc, msg)
    # slam_fs_create's own cases
    for n in (0, -1, (1 << 24) + 1):
        rc, msg = create(_cfg(), _acfg(), _pcfg(), n, 8)
        assert rc == SLAM_ERR_ARG and "n_particles" in msg, (n, rc, msg)
    rc, msg = create(_cfg(r_dist=0.0), _acfg(), _pcfg(), 100, 8)
    assert rc == SLAM_ERR_ARG and "r_dist" in msg, (rc, msg)
    rc, msg = create(_cfg(r_dir=0.0), _acfg(), _pcfg(), 100, 8)
    assert rc == SLAM_ERR_ARG and "r_dir" in msg, (rc, msg)


def test_the_binding_knows_the_symbol(lib):
    from slamhip import _lib
    assert "slam_fs_create_assoc_proposal" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["slam_fs_create_assoc_proposal"]
    assert res is C.c_int and len(args) == 7
    assert hasattr(lib, "slam_fs_create_assoc_proposal")
    assert _lib.FS_PROPOSAL == ("motion", "measurement")


def test_front_end_argument_errors():
    from slamhip.fastslam import DeviceFastSLAM
    with pytest.raises(ValueError, match="proposal"):
        DeviceFastSLAM(10, 3, association="ml_marginal")
    with pytest.raises(ValueError, match="proposal"):
        DeviceFastSLAM(10, 3, association="ml_marginal", proposal="motion")
    with pytest.raises(ValueError, match="ml_marginal"):
        DeviceFastSLAM(10, 3, association="ml", proposal="measurement")
    with pytest.raises(ValueError, match="association"):
        DeviceFastSLAM(10, 3, association="nearest")
    with pytest.raises(ValueError, match="p_new"):
        DeviceFastSLAM(10, 3, association="ml_marginal", proposal="measurement", p_new=0.0)
