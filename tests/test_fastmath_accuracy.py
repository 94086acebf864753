"""The host restatements of csrc/fastmath.hpp (tests/fastmath_ref.py) within
the header's own accuracy claims, against the 200-bit references of
tests/golden/fastmath.npz (tools/gen_fastmath_golden.py), on the argument sets
tests/test_gpu_fastmath.py runs on the device.  With that test's bit equality:
device = restatement, and restatement within its bound.

"measured" below: the worst error of the restatement on these sets (exact
fmas, mpmath reference), in the unit the assertion uses."""
import math
import pathlib
import sys
from fractions import Fraction

import numpy as np
import pytest

import fastmath_ref as fr
from conftest import golden

mp = pytest.importorskip("mpmath")
ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import gen_fastmath_golden as gen  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    g = golden("fastmath")
    return {k: g[k] for k in g.files}


def worst_sincos(got, ref, floor=0.0, rows=None):
    """Worst error of n x 2 (sin, cos) against n x 4 (s_hi, s_lo, c_hi, c_lo), in ulp of
    max(|value|, floor)."""
    w = 0.0
    for i in (range(len(got)) if rows is None else rows):
        w = max(w, fr.ulp_err(got[i, 0], ref[i, 0], ref[i, 1], floor),
                fr.ulp_err(got[i, 1], ref[i, 2], ref[i, 3], floor))
    return w


def test_fixture_matches_its_generator(gold):
    """Shapes follow the argument sets, the searched arguments are the search's, and
    every 23rd reference recomputes to the committed bits."""
    hard = gold["fast_sincos_hard"]
    assert np.array_equal(hard, fr.hard_sincos_search()) and hard.size == 200
    sets = {
        "fast_sincos_ref": (gen.ref_sincos, fr.args_fast_sincos(hard)),
        "handoff_ref": (gen.ref_sincos, gold["handoff_args"]),
        "small_sincos_ref": (gen.ref_sincos, fr.args_small_sincos()),
        "heading_sincos_tab_ref": (gen.ref_sincos, fr.args_heading_sincos_tab()),
        "rotate_sc_ref": (gen.ref_rotate, fr.args_rotate_sc()),
        "exp_ref": (gen.ref_exp, fr.args_exp()),
        "exp_nhalf_ref": (lambda a: gen.ref_exp(a, -0.5), fr.args_exp_nhalf()),
        "rng_log_ref": (gen.ref_rng_log, fr.args_rng_log_words()),
        "rng_sincos_ref": (gen.ref_rng_sincos, fr.args_rng_sincos_words()),
    }
    assert np.array_equal(gold["rng_log_scaled_d"], fr.args_rng_log_words() + 1.0)
    assert np.array_equal(gold["handoff_args"], fr.args_sincos_handoff(), equal_nan=True)
    for key, (fn, args) in sets.items():
        assert gold[key].shape[0] == len(args), key
        assert fr.same_bits(fn(args[::23]), gold[key][::23]).all(), key


def test_fast_sincos(gold):
    """< 1 ulp of max(|value|, 2^-35) everywhere (measured 0.67; 0.25 on the 200 doubles
    closest to a multiple of pi/2).  In plain ulp those 200 exceed 1 (measured 4.8e4 at
    321307.9594422229): y = fma(-n, kPio2Mid, r1 - r) forms r1 - r with a rounding when
    |r| << |r1|, an absolute error below 2^-89 -- the header's corrected claim."""
    hard = gold["fast_sincos_hard"]
    xs = fr.args_fast_sincos(hard)
    got = fr.evaluate("fast_sincos", fr.pad4(xs))
    ref = gold["fast_sincos_ref"]
    rows_hard = range(len(xs) - len(hard), len(xs))
    assert np.array_equal(xs[len(xs) - len(hard):], hard)
    w = worst_sincos(got, ref, 2.0 ** -35)
    wh = worst_sincos(got, ref, 2.0 ** -35, rows_hard)
    plain = worst_sincos(got, ref, 0.0, rows_hard)
    print(f"fast_sincos: {w:.3g} ulp of max(|v|, 2^-35), hard set {wh:.3g}; hard set in plain ulp {plain:.3g}")
    assert w < 1.0, w
    assert plain > 1.0, plain


def test_small_sincos(gold):
    """< 1 ulp (measured 0.69)."""
    got = fr.evaluate("small_sincos", fr.pad4(fr.args_small_sincos()))
    w = worst_sincos(got, gold["small_sincos_ref"])
    print(f"small_sincos: {w:.3g} ulp")
    assert w < 1.0, w


def test_rotate_sc(gold):
    """Two roundings per component: the inner product's (half an ulp of it) and the
    fma's (half an ulp of the result)."""
    a = fr.args_rotate_sc()
    got = fr.evaluate("rotate_sc", a)
    ref = gold["rotate_sc_ref"]
    for i in range(len(a)):
        s, c, sd, cd = (float(v) for v in a[i])
        for k, inner in ((0, c * sd), (1, s * sd)):
            err = abs(Fraction(float(got[i, k])) - fr.dd(ref[i, 2 * k], ref[i, 2 * k + 1]))
            assert err <= Fraction(math.ulp(inner)) / 2 + Fraction(math.ulp(ref[i, 2 * k])) / 2, (i, k)


def test_heading_sincos_tab(gold):
    """<= 2 ulp of max(|value|, 2^-20), the bar of tests/test_heading_sincos.py, on the
    device test's arguments (the two beyond 3.2415926535897931 take fast_sincos)."""
    got = fr.evaluate("heading_sincos_tab", fr.pad4(fr.args_heading_sincos_tab()))
    w = worst_sincos(got, gold["heading_sincos_tab_ref"], 2.0 ** -20)
    print(f"heading_sincos_tab: {w:.3g} ulp of max(|v|, 2^-20)")
    assert w <= 2.0, w


def _exp_errors(name, xs, ref, scale):
    """(worst on normal results, worst on subnormal results in units of 2^-1074); zero and
    infinite results must be the reference's."""
    got = fr.evaluate(name, fr.pad4(xs))[:, 0]
    wn = ws = 0.0
    exp200 = mp.workprec(200)(lambda x: mp.exp(mp.mpf(float(x)) * scale))
    for x, g, (hi, lo) in zip(xs, got, ref):
        if np.isnan(x):
            assert np.isnan(g)
        elif np.isinf(hi):
            assert g == hi, (x, g)
        elif abs(hi) >= 2.0 ** -1022:
            wn = max(wn, fr.ulp_err(g, hi, lo))
        else:       # subnormal or zero: the fixture's lo cannot hold the tail there
            true = gen.to_fraction(exp200(x)) if np.isfinite(x) else Fraction(0)
            ws = max(ws, float(abs(Fraction(float(g)) - true) / Fraction(2.0 ** -1074)))
    return wn, ws


def test_exp_lean(gold):
    """< 1 ulp on normal results (measured 0.75); at most 1 ulp of the true value on
    subnormal results, where the ldexp is a second rounding (measured 0.50, which shows as
    1 ulp against the correctly rounded double)."""
    wn, ws = _exp_errors("exp_lean", fr.args_exp(), gold["exp_ref"], 1.0)
    print(f"exp_lean: normal {wn:.3g} ulp, subnormal {ws:.3g} ulp")
    assert wn < 1.0, wn
    assert ws <= 1.0, ws


@pytest.mark.parametrize("name", ["exp_tab", "exp_nhalf"])
def test_exp_tab_and_nhalf(gold, name):
    """The header's "under 0.9 ulp" (the bar of tests/test_exp_tab.py) on the device
    test's arguments, normal results."""
    if name == "exp_tab":
        wn, ws = _exp_errors(name, fr.args_exp(), gold["exp_ref"], 1.0)
    else:
        wn, ws = _exp_errors(name, fr.args_exp_nhalf(), gold["exp_nhalf_ref"], -0.5)
    print(f"{name}: normal {wn:.3g} ulp, subnormal {ws:.3g} ulp")
    assert wn < 0.9, wn


def test_rng_log_tab(gold):
    """<= 1.3 ulp, the header's claim (measured 1.21, at a slot edge); exactly +0 at word 2^32 - 1."""
    words = fr.args_rng_log_words()
    got = fr.evaluate("rng_log_tab", fr.pad4(words))[:, 0]
    ref = gold["rng_log_ref"]
    w = max(fr.ulp_err(g, hi, lo) for g, (hi, lo) in zip(got, ref))
    print(f"rng_log_tab: {w:.3g} ulp")
    assert w <= 1.3, w
    last = got[words == 2.0 ** 32 - 1]
    assert last.size and np.all(last == 0.0) and not np.signbit(last).any()


def test_rng_sincos2pi_tab(gold):
    """< 1.5 ulp of 1: an absolute error below 1.5 2^-53 (measured 1.25 2^-53)."""
    got = fr.evaluate("rng_sincos2pi_tab", fr.pad4(fr.args_rng_sincos_words()))
    ref = gold["rng_sincos_ref"]
    w = 0.0
    for g, r in zip(got, ref):
        for k in (0, 1):
            w = max(w, float(abs(Fraction(float(g[k])) - fr.dd(r[2 * k], r[2 * k + 1])) / Fraction(2.0 ** -53)))
    print(f"rng_sincos2pi_tab: {w:.3g} ulp of 1")
    assert w < 1.5, w


def test_rng_sincos2pi(gold):
    """The A/B form's "a few ulp": measured 1.56 ulp of the value over the word set (the
    one rounding of t = r pi/2 carries through sin beside its zeros), asserted at the
    next half ulp above, 2.0."""
    got = fr.evaluate("rng_sincos2pi", fr.pad4(fr.args_rng_sincos_words()))
    w = worst_sincos(got, gold["rng_sincos_ref"])
    print(f"rng_sincos2pi: {w:.3g} ulp")
    assert w <= 2.0, w
