"""Landmark evidence and removal, C-ABI and front end, CPU side: the exports
exist, slam_fs_prune_config in the binding has the header's layout,
slam_fs_check_prune_config rejects each bad field (host only, no device needed)
and NULL handles are argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import PKG  # noqa: F401  (puts the package on sys.path)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("slam_fs_check_prune_config", "slam_fs_set_pruning", "slam_fs_set_evidence",
           "slam_fs_get_evidence", "slam_fs_get_removed")


@pytest.fixture(scope="module")
def lib():
    from slamhip import _lib
    return _lib.load()


def _cfg(**kw):
    from slamhip.fastslam import prune_config
    c = prune_config(7.2, view_angle=np.deg2rad(80.0), ev_max=5)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_the_exports_exist_and_the_binding_knows_them(lib):
    from slamhip import _lib
    for name in EXPORTS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name][0] is C.c_int


def test_struct_layout_matches_the_header():
    from slamhip._lib import FSPruneConfig
    text = open(os.path.join(ROOT, "include", "slam_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} slam_fs_prune_config;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(double|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    assert [n for n, _ in FSPruneConfig._fields_] == [n for n, _ in fields]
    size = {"double": 8, "int32_t": 4}
    off = 0
    for name, ctype in fields:
        f = getattr(FSPruneConfig, name)
        assert (f.offset, f.size) == (off, size[ctype]), name
        off += size[ctype]
    assert C.sizeof(FSPruneConfig) == off == 40


def test_check_prune_config_rejects_each_bad_field(lib):
    from slamhip._lib import SLAM_ERR_ARG, SLAM_OK

    def chk(c):
        rc = lib.slam_fs_check_prune_config(None if c is None else C.byref(c))
        return rc, lib.slam_last_error().decode()

    assert chk(_cfg())[0] == SLAM_OK
    assert chk(_cfg(use_angle=0, view_tan=np.nan))[0] == SLAM_OK      # unused without the angle
    assert chk(_cfg(init=0, remove_below=0, ev_max=0, hit=0, miss=0))[0] == SLAM_OK
    rc, msg = chk(None)
    assert rc == SLAM_ERR_ARG and "NULL" in msg
    for bad in (0.0, -1.0, np.inf, -np.inf, np.nan):
        rc, msg = chk(_cfg(view_range=bad))
        assert rc == SLAM_ERR_ARG and "view_range" in msg, (bad, rc, msg)
    rc, msg = chk(_cfg(view_tan=np.nan))
    assert rc == SLAM_ERR_ARG and "view_tan" in msg, (rc, msg)
    for k in ("hit", "miss"):
        rc, msg = chk(_cfg(**{k: -1}))
        assert rc == SLAM_ERR_ARG and k in msg, (k, rc, msg)
    rc, msg = chk(_cfg(init=6))                                       # ev_max = 5
    assert rc == SLAM_ERR_ARG and "ev_max" in msg, (rc, msg)
    rc, msg = chk(_cfg(init=1, remove_below=2))
    assert rc == SLAM_ERR_ARG and "remove_below" in msg, (rc, msg)


def test_null_handles_are_argument_errors(lib):
    from slamhip._lib import SLAM_ERR_ARG
    buf = (C.c_int32 * 4)()
    c = _cfg()
    assert lib.slam_fs_set_pruning(None, C.byref(c)) == SLAM_ERR_ARG
    assert lib.slam_fs_set_pruning(None, None) == SLAM_ERR_ARG
    for name in ("slam_fs_set_evidence", "slam_fs_get_evidence", "slam_fs_get_removed"):
        assert getattr(lib, name)(None, buf) == SLAM_ERR_ARG, name
        assert "NULL" in lib.slam_last_error().decode()


def test_front_end_config_and_argument_errors():
    from slamhip.fastslam import DeviceFastSLAM, prune_config
    c = prune_config(7.2)
    assert (c.view_range, c.use_angle, c.init, c.hit, c.miss, c.remove_below) == (7.2, 0, 1, 1, 1, 0)
    assert c.ev_max == 2 ** 31 - 1
    a = np.deg2rad(80.0)
    c = prune_config(11.0, view_angle=a, init=2, hit=3, miss=4, ev_max=9, remove_below=1)
    assert c.use_angle == 1 and c.view_tan == float(np.tan(np.pi / 2 - a))
    assert (c.init, c.hit, c.miss, c.ev_max, c.remove_below) == (2, 3, 4, 9, 1)
    with pytest.raises(ValueError, match="prune"):
        DeviceFastSLAM(10, 3, prune=dict(view_range=7.2))             # known association
