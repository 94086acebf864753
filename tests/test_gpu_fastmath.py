"""The compiled device code of csrc/fastmath.hpp's routines, run one lane per
argument through slam_debug_math (csrc/math_debug_api.hip: the very inline
functions the production kernels call, tables staged in LDS as production
stages them), against the host restatements of tests/fastmath_ref.py.

Every routine without an approximate hardware instruction must give the
restatement's 64-bit patterns: no tolerance, -0.0 is not +0.0, a NaN matches
any NaN.  That pins the fma_k / fma_kk inline assembly, the 1.5 2^52 shift read
from kdm's low word, v_ldexp_f64 into the subnormals, the frexp builtins, the
LDS staging of the three tables and the range selects.  The restatements are
held to the header's accuracy claims against mpmath on the same argument sets
in tests/test_fastmath_accuracy.py (device = restatement, restatement within
its bound).  sqrt_pos and rng_log_scaled start from v_rsq_f64 / v_rcp_f64 seeds
and the fast_sincos hand-off goes to the device library: those three are held
to a correctly rounded reference (np.sqrt, tests/golden/fastmath.npz).

Needs NumPy and the standard library only; argument sets are seeded
(fastmath_ref.args_*)."""
import ctypes as C

import numpy as np
import pytest

import fastmath_ref as fr
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    g = golden("fastmath")
    return {k: g[k] for k in g.files}


def device(name, args):
    from slamhip import _lib
    a = np.ascontiguousarray(fr.pad4(args))
    out = np.full((a.shape[0], 2), np.nan)
    p = C.POINTER(C.c_double)
    _lib.check(_lib.load().slam_debug_math(0, _lib.MATH_FN[name], a.shape[0], a.ctypes.data_as(p),
                                           out.ctypes.data_as(p)), "slam_debug_math")
    return out


def assert_bits(name, args, ncol):
    args = np.asarray(args)
    dev = device(name, args)[:, :ncol]
    ref = fr.evaluate(name, fr.pad4(args))[:, :ncol]
    ok = fr.same_bits(dev, ref).all(axis=1)
    if not ok.all():
        bad = np.flatnonzero(~ok)
        lines = [f"{name}: {bad.size} of {ok.size} arguments differ"]
        for i in bad[:8]:
            lines.append(f"  arg {[float(v).hex() for v in np.atleast_1d(args[i])]} "
                         f"device {[float(v).hex() for v in dev[i]]} "
                         f"restatement {[float(v).hex() for v in ref[i]]}")
        raise AssertionError("\n".join(lines))
    return dev


def test_fast_sincos_bits(gold):
    """|x| < 2^19: random in +-8 and +-2^19, k pi/2 and its neighbours, the last double
    below 2^19, the 200 doubles closest to a multiple of pi/2, zeros and denormals."""
    assert_bits("fast_sincos", fr.args_fast_sincos(gold["fast_sincos_hard"]), 2)


def test_small_sincos_bits():
    assert_bits("small_sincos", fr.args_small_sincos(), 2)


def test_rotate_sc_bits():
    assert_bits("rotate_sc", fr.args_rotate_sc(), 2)


def test_heading_sincos_tab_bits():
    assert_bits("heading_sincos_tab", fr.args_heading_sincos_tab(), 2)


def test_exp_lean_bits():
    assert_bits("exp_lean", fr.args_exp(), 1)


def test_exp_tab_bits():
    assert_bits("exp_tab", fr.args_exp(), 1)


def test_exp_tab_nonpos_bits():
    assert_bits("exp_tab_nonpos", fr.args_exp(nonpos=True), 1)


def test_exp_nhalf_bits():
    """exp_nhalf<false> against its restatement, and on the device against
    exp_tab(-y/2)'s bits (the claim tests/test_exp_tab.py checks on the host)."""
    ys = fr.args_exp_nhalf()
    dev = assert_bits("exp_nhalf", ys, 1)
    tab = device("exp_tab", -ys * 0.5)[:, :1]
    ok = fr.same_bits(dev, tab)[:, 0]
    assert ok.all(), [(float(y).hex(), float(a).hex(), float(b).hex())
                      for y, a, b in zip(ys[~ok][:8], dev[~ok][:8, 0], tab[~ok][:8, 0])]


def test_exp_nhalf_nonpos_bits():
    ys = fr.args_exp_nhalf(nonpos=True)
    dev = assert_bits("exp_nhalf_nonpos", ys, 1)
    tab = device("exp_tab_nonpos", -ys * 0.5)[:, :1]
    assert fr.same_bits(dev, tab).all()


def test_rng_log_tab_bits():
    words = fr.args_rng_log_words()
    dev = assert_bits("rng_log_tab", words, 1)
    last = dev[words == 2.0 ** 32 - 1, 0]
    assert last.size and np.all(last == 0.0) and not np.signbit(last).any()     # log(1) = +0.0


def test_rng_sincos2pi_tab_bits():
    assert_bits("rng_sincos2pi_tab", fr.args_rng_sincos_words(), 2)


def test_rng_sincos2pi_bits():
    assert_bits("rng_sincos2pi", fr.args_rng_sincos_words(), 2)


def test_sqrt_pos_against_correctly_rounded():
    """sqrt_pos (v_rsq_f64 seed, no bits to restate) against np.sqrt: within 1 ulp
    everywhere -- the last Newton step on a value already good to 2^-50 is a faithful
    rounding -- sqrt_pos(0) = 0, and equal bits for x >= 2^-960: below that the residual
    fma(-g, g, x) drops under the normal range and the last step need no longer correct.
    Measured: all 4,289 arguments from 2^-960 up, and the ones below it, have np.sqrt's bits
    (the header's "refinement of the device library's sqrt" holds as worded)."""
    xs = fr.args_sqrt_pos()
    dev = device("sqrt_pos", xs)[:, 0]
    ref = np.sqrt(xs)
    assert dev[xs == 0.0].size and np.all(dev[xs == 0.0] == 0.0)
    err = np.abs(dev - ref) / np.spacing(ref)
    err[xs == 0.0] = 0.0
    big = xs >= 2.0 ** -960
    differ = ~fr.same_bits(dev, ref) & big
    print(f"sqrt_pos: worst {err.max():.3g} ulp; {differ.sum()} of {big.sum()} differ from np.sqrt above 2^-960")
    assert err.max() <= 1.0, float(err.max())
    assert not differ.any(), [float(x).hex() for x in xs[differ][:8]]


def test_rng_log_scaled_within_1ulp(gold):
    """rng_log_scaled(d, -32) (v_rcp_f64 seed) within the header's 1 ulp of
    log(d 2^-32), d = word + 1 over rng_log_tab's words; exactly 0 at d = 2^32.
    Measured worst: 0.72 ulp."""
    d = gold["rng_log_scaled_d"]
    dev = device("rng_log_scaled", np.stack([d, np.full_like(d, -32.0)], axis=1))[:, 0]
    ref = gold["rng_log_ref"]
    err = np.array([fr.ulp_err(v, h, lo) if h != 0.0 else abs(v) for v, (h, lo) in zip(dev, ref)])
    print(f"rng_log_scaled: worst {err.max():.3g} ulp")
    assert np.all(dev[d == 2.0 ** 32] == 0.0) and (d == 2.0 ** 32).any()
    assert err.max() <= 1.0, float(err.max())


def test_fast_sincos_handoff(gold):
    """|x| >= 2^19, inf and NaN take the device library's sincos: within 2 ulp of
    sin / cos, NaN for +-inf and NaN.  The point is that the branch is taken and selects
    nothing wrong, not the library's accuracy.  Measured worst: 0.49 ulp."""
    xs, ref = gold["handoff_args"], gold["handoff_ref"]
    assert np.array_equal(xs, fr.args_sincos_handoff(), equal_nan=True)
    dev = device("fast_sincos", xs)
    fin = np.isfinite(xs)
    assert (~fin).sum() == 3 and np.isnan(dev[~fin]).all()
    worst = 0.0
    for (s, c), (sh, sl, ch, cl) in zip(dev[fin], ref[fin]):
        worst = max(worst, fr.ulp_err(s, sh, sl), fr.ulp_err(c, ch, cl))
    print(f"fast_sincos hand-off: worst {worst:.3g} ulp")
    assert worst <= 2.0, worst
