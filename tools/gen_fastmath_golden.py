"""Generate tests/golden/fastmath.npz with mpmath at 200 bits: the argument
sets of the fastmath.hpp tests that need a high-precision search or reference
(the fast_sincos arguments closest to a multiple of pi/2, the library hand-off
set, the rng_log_scaled set) and, for every argument set of
tests/test_gpu_fastmath.py, the correctly rounded result as a double-double
(hi, lo).  tests/test_fastmath_accuracy.py recomputes a sample of it.

    python tools/gen_fastmath_golden.py       # writes tests/golden/fastmath.npz

Fixed seeds (tests/fastmath_ref.py) and fixed archive timestamps: a second run
reproduces the file byte for byte.
"""
import io
import pathlib
import sys
import zipfile
from fractions import Fraction

import mpmath as mp
import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import fastmath_ref as fr  # noqa: E402

PREC = 200            # every reference below is formed at this precision, whatever the caller's
OUT = ROOT / "tests/golden/fastmath.npz"


def to_fraction(v):
    """An mpf's exact value."""
    sign, man, exp, _ = v._mpf_
    f = Fraction(int(man)) * Fraction(2) ** int(exp)
    return -f if sign else f


def split(v):
    """The 200-bit value v as (hi, lo): hi the nearest double, lo the nearest double of the rest."""
    if mp.isnan(v):
        return np.nan, np.nan
    if mp.isinf(v):
        return (np.inf if v > 0 else -np.inf), 0.0
    f = to_fraction(mp.mpf(v))
    try:
        hi = float(f)
    except OverflowError:
        return (np.inf if f > 0 else -np.inf), 0.0
    return hi, float(f - Fraction(hi))


def _finite(fn, x):
    x = float(x)
    if np.isnan(x):
        return mp.nan
    return fn(x)


@mp.workprec(PREC)
def ref_sincos(xs):
    """sin and cos of each double: n x 4 (s_hi, s_lo, c_hi, c_lo); NaN for inf / NaN."""
    out = np.empty((len(xs), 4))
    for i, x in enumerate(xs):
        if not np.isfinite(x):
            out[i] = np.nan
            continue
        out[i] = split(mp.sin(mp.mpf(float(x)))) + split(mp.cos(mp.mpf(float(x))))
    return out


@mp.workprec(PREC)
def ref_exp(xs, scale=1.0):
    """exp(scale x): n x 2."""
    def f(x):
        if x == np.inf * scale:
            return mp.inf
        if x == -np.inf * scale:
            return mp.mpf(0)
        return mp.exp(mp.mpf(x) * scale)
    return np.array([split(_finite(f, x)) for x in xs])


def ref_rotate(rows):
    """The exact s cd + c sd and c cd - s sd of the four doubles: n x 4."""
    out = np.empty((len(rows), 4))
    for i, (s, c, sd, cd) in enumerate(rows):
        s, c, sd, cd = (Fraction(float(v)) for v in (s, c, sd, cd))
        so, co = s * cd + c * sd, c * cd - s * sd
        hs, hc = float(so), float(co)
        out[i] = (hs, float(so - Fraction(hs)), hc, float(co - Fraction(hc)))
    return out


@mp.workprec(PREC)
def ref_rng_log(words):
    """log((word + 1) 2^-32): n x 2 (exactly 0 at word 2^32 - 1)."""
    return np.array([split(mp.log(mp.mpf(int(w) + 1) / 2 ** 32)) for w in words])


@mp.workprec(PREC)
def ref_rng_sincos(words):
    """sin, cos of 2 pi (word + 1) 2^-32: n x 4, exact at the quarter turns."""
    exact = {0: (0.0, 1.0), 1: (1.0, 0.0), 2: (0.0, -1.0), 3: (-1.0, 0.0)}
    out = np.empty((len(words), 4))
    for i, w in enumerate(words):
        B = (int(w) + 1) % 2 ** 32
        if B % 2 ** 30 == 0:
            s, c = exact[B >> 30]
            out[i] = (s, 0.0, c, 0.0)
            continue
        a = 2 * mp.pi * B / 2 ** 32
        out[i] = split(mp.sin(a)) + split(mp.cos(a))
    return out


def build():
    hard = fr.hard_sincos_search()
    handoff = fr.args_sincos_handoff()
    log_words = fr.args_rng_log_words()
    return {
        "fast_sincos_hard": hard,
        "fast_sincos_ref": ref_sincos(fr.args_fast_sincos(hard)),
        "handoff_args": handoff,
        "handoff_ref": ref_sincos(handoff),
        "small_sincos_ref": ref_sincos(fr.args_small_sincos()),
        "heading_sincos_tab_ref": ref_sincos(fr.args_heading_sincos_tab()),
        "rotate_sc_ref": ref_rotate(fr.args_rotate_sc()),
        "exp_ref": ref_exp(fr.args_exp()),
        "exp_nhalf_ref": ref_exp(fr.args_exp_nhalf(), -0.5),
        "rng_log_scaled_d": log_words + 1.0,
        "rng_log_ref": ref_rng_log(log_words),
        "rng_sincos_ref": ref_rng_sincos(fr.args_rng_sincos_words()),
    }


def write(path, arrays):
    """An .npz np.load reads, with constant member timestamps."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    arrays = build()
    write(OUT, arrays)
    print(OUT, OUT.stat().st_size, "bytes;", {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main()
