"""EKF-SLAM landmark evidence and removal, C-ABI and front end, CPU side: the
header's new symbols are exported and bound, slam_ekfslam_prune_info_t in the
binding has the header's layout, the configuration is FastSLAM's, and every
argument error that needs no device is returned on NULL handles."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import PKG  # noqa: F401  (puts the package on sys.path)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("slam_ekfslam_set_pruning", "slam_ekfslam_set_evidence", "slam_ekfslam_get_evidence",
           "slam_ekfslam_remove", "slam_ekfslam_prune_info")


@pytest.fixture(scope="module")
def lib():
    from slamhip import _lib
    return _lib.load()


def test_the_exports_exist_and_the_binding_knows_them(lib):
    from slamhip import _lib
    text = open(os.path.join(ROOT, "include", "slam_hip.h")).read()
    for name in EXPORTS:
        assert re.search(r"^int %s\(slam_ekfslam\* h" % name, text, flags=re.M), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name][0] is C.c_int
    # both estimators take the same configuration
    assert _lib.SIGNATURES["slam_ekfslam_set_pruning"][1] == _lib.SIGNATURES["slam_fs_set_pruning"][1]
    assert "const slam_fs_prune_config* cfg);" in text.split("int slam_ekfslam_set_pruning(")[1][:80]


def test_prune_info_layout_matches_the_header():
    from slamhip._lib import EKFSLAMPruneInfo
    text = open(os.path.join(ROOT, "include", "slam_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} slam_ekfslam_prune_info_t;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(double|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    assert [n for n, _ in EKFSLAMPruneInfo._fields_] == [n for n, _ in fields]
    size = {"double": 8, "int32_t": 4}
    off = 0
    for name, ctype in fields:
        f = getattr(EKFSLAMPruneInfo, name)
        assert (f.offset, f.size) == (off, size[ctype]), name
        off += size[ctype]
    assert C.sizeof(EKFSLAMPruneInfo) == off == 32


def test_null_handles_are_argument_errors(lib):
    from slamhip._lib import SLAM_ERR_ARG, EKFSLAMPruneInfo
    from slamhip.fastslam import prune_config
    buf = (C.c_int32 * 4)()
    c = prune_config(7.2, view_angle=np.deg2rad(80.0), ev_max=5)
    assert lib.slam_ekfslam_set_pruning(None, C.byref(c)) == SLAM_ERR_ARG
    assert "NULL" in lib.slam_last_error().decode()
    assert lib.slam_ekfslam_set_pruning(None, None) == SLAM_ERR_ARG
    for name in ("slam_ekfslam_set_evidence", "slam_ekfslam_get_evidence"):
        assert getattr(lib, name)(None, buf) == SLAM_ERR_ARG, name
        assert "NULL" in lib.slam_last_error().decode()
    assert lib.slam_ekfslam_remove(None, 1, buf) == SLAM_ERR_ARG
    assert lib.slam_ekfslam_remove(None, 0, None) == SLAM_ERR_ARG
    assert "NULL" in lib.slam_last_error().decode()
    info = EKFSLAMPruneInfo()
    assert lib.slam_ekfslam_prune_info(None, C.byref(info)) == SLAM_ERR_ARG
    assert "NULL" in lib.slam_last_error().decode()


def test_front_end_shares_the_configuration_and_rejects_known_ids():
    import inspect

    import slamhip.ekf as ekf
    import slamhip.fastslam as fs
    assert ekf.prune_config is fs.prune_config
    for name in ("set_pruning", "evidence", "set_evidence", "remove", "prune_info"):
        assert callable(getattr(ekf.DeviceEKFSLAM, name)), name
    assert "prune" in inspect.signature(ekf.DeviceEKFSLAM.__init__).parameters
    with pytest.raises(ValueError, match="prune"):
        ekf.DeviceEKFSLAM(10, prune=dict(view_range=7.2))             # known ids: before any device call
