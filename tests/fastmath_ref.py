"""Host restatements of csrc/fastmath.hpp, operation by operation, and the
argument sets the device and accuracy tests share.

Every fma is exact (rational arithmetic, one rounding); every other operation
is an IEEE double; ldexp is math.ldexp, rint is np.rint, the frexp pair is
math.frexp.  Tables are read out of the header; constants are written out
literally.  Every branch of the device code is restated, range selects
included; where the device hands an argument to the device library's sincos
the restatement takes the C library's (not bit-comparable: the tests hold that
branch to a bound, not to bits).

Used by tests/test_gpu_fastmath.py (device bits = these bits), by
tests/test_fastmath_accuracy.py (these within the header's claims, against
mpmath), by tests/test_exp_tab.py and tests/test_heading_sincos.py, and by
tools/gen_fastmath_golden.py (the references of tests/golden/fastmath.npz).
"""
import math
import pathlib
import re
import struct
from fractions import Fraction

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
HEADER = ROOT / "slam-robot_simu_amd/csrc/fastmath.hpp"
HEX = r"-?0x[0-9a-fA-F.]+p[-+]?\d+"
INF, NAN = math.inf, math.nan


# ----------------------------------------------------------------- tables
def _table(name, n):
    src = HEADER.read_text()
    m = re.search(name + r"\[%d\] = \{(.*?)\n\};" % n, src, re.S)
    assert m, name
    return [float.fromhex(x) for x in re.findall(HEX, m.group(1))]


def exp_table():
    v = _table("kExpTab64", 64)
    return list(zip(v[0::2], v[1::2]))


def sincos_table():
    v = _table("kRngSinCos256", 256)
    return [(v[2 * k], v[2 * k + 1]) for k in range(256)]


class RngTabs:
    """RngTabs of the header: sc (sin, cos)(2 pi j / 256), li (invc, -log(invc) hi), ll its lo."""

    def __init__(self):
        self.sc = sincos_table()
        v = _table("kRngLogInvHi", 256)
        self.li = [(v[2 * k], v[2 * k + 1]) for k in range(256)]
        self.ll = _table("kRngLogLo", 256)
        assert len(self.sc) == 256 and len(self.li) == 256 and len(self.ll) == 256


# ------------------------------------------------------------- primitives
def fma(a, b, c):
    """a b + c with one rounding (IEEE fusedMultiplyAdd, signed zeros included)."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c                          # NaN / inf: the two-step form decides the same
    p = Fraction(a) * Fraction(b)
    s = p + Fraction(c)
    if s == 0:
        # exact zero: (+-0) + (+-0) by the sum's rule, an exact cancellation is +0
        return a * b + c if p == 0 else 0.0
    try:
        return float(s)
    except OverflowError:
        return math.copysign(INF, s)


def ldexp(v, k):
    try:
        return math.ldexp(v, k)
    except OverflowError:
        return math.copysign(INF, v)


def rint(x):
    return float(np.rint(x))


def fmin(a, b):
    return b if a != a else (a if b != b else min(a, b))


def fmax(a, b):
    return b if a != a else (a if b != b else max(a, b))


def bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def low_word_int(x):
    """(int)(uint32_t)__double_as_longlong(x): the low 32 bits read as a signed int."""
    w = bits(x) & 0xFFFFFFFF
    return w - (1 << 32) if w & 0x80000000 else w


def lib_sincos(x):
    """Stand-in for the device library's sincos (the hand-off branch)."""
    if not math.isfinite(x):
        return NAN, NAN
    return math.sin(x), math.cos(x)


# ---------------------------------------------------------------- sin/cos
K_INV_PIO2 = 6.36619772367581382433e-01
K_PIO2_HI = 1.57079632679489655800e+00
K_PIO2_MID = 6.12323399573676603587e-17
K_PIO2_LO = -1.49738490485916983e-33
K_PIO4 = 7.85398163397448278999e-01
S1, S2, S3 = -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04
S4, S5, S6 = 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10
C1, C2, C3 = 4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05
C4, C5, C6 = -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11


def ksin(x, y):
    z = x * x
    v = z * x
    r = fma(z, fma(z, fma(z, fma(z, S6, S5), S4), S3), S2)
    return x - ((z * (0.5 * y - v * r) - y) - v * S1)


def ksin0(x):
    z = x * x
    v = z * x
    r = fma(z, fma(z, fma(z, fma(z, S6, S5), S4), S3), S2)
    return x + v * fma(z, r, S1)


def kcos(x, y):
    z = x * x
    w2 = z * z
    r = z * fma(z, fma(z, C3, C2), C1) + w2 * w2 * fma(z, fma(z, C6, C5), C4)
    hz = 0.5 * z
    w = 1.0 - hz
    return w + (((1.0 - w) - hz) + (z * r - x * y))


def _quadrant(n, s, c):
    q = int(n) & 3
    sa = c if q & 1 else s
    ca = s if q & 1 else c
    return (-sa if q & 2 else sa), (-ca if (q + 1) & 2 else ca)


def fast_sincos(x):
    if not (abs(x) < 2.0 ** 19):
        return lib_sincos(x)
    n = rint(x * K_INV_PIO2)
    r1 = fma(-n, K_PIO2_HI, x)
    r = fma(-n, K_PIO2_MID, r1)
    y = fma(-n, K_PIO2_MID, r1 - r)
    y = fma(-n, K_PIO2_LO, y)
    return _quadrant(n, ksin(r, y), kcos(r, y))


def small_sincos(x):
    if abs(x) <= 0.0625:
        z = x * x
        ps = fma(z, fma(z, fma(z, 1.0 / 362880.0, -1.0 / 5040.0), 1.0 / 120.0), -1.0 / 6.0)
        s = fma(x * z, ps, x)
        pc = fma(z, fma(z, fma(z, 1.0 / 40320.0, -1.0 / 720.0), 1.0 / 24.0), -0.5)
        return s, fma(z, pc, 1.0)
    if abs(x) <= K_PIO4:
        return ksin0(x), kcos(x, 0.0)
    return fast_sincos(x)


def rotate_sc(s, c, sd, cd):
    return fma(s, cd, c * sd), fma(c, cd, -(s * sd))


def heading_sincos_tab(x, T):
    """T: the (sin, cos) table (sincos_table()) or an RngTabs."""
    sc = T.sc if isinstance(T, RngTabs) else T
    k128pi = 40.74366543152521
    hi, lo = float.fromhex("0x1.921fb54442dp-6"), float.fromhex("0x1.8469898cc5170p-54")
    if not (abs(x) <= 3.2415926535897931):
        return fast_sincos(x)
    j = rint(x * k128pi)
    r = fma(-j, lo, fma(-j, hi, x))
    ts, tc = sc[int(j) & 255]
    z = r * r
    sr = fma(r * z, fma(z, fma(z, -1.0 / 5040.0, 1.0 / 120.0), -1.0 / 6.0), r)
    cr = fma(z, fma(z, fma(z, -1.0 / 720.0, 1.0 / 24.0), -0.5), 1.0)
    return fma(ts, cr, tc * sr), fma(tc, cr, -(ts * sr))


# -------------------------------------------------------------------- exp
def exp_lean(x):
    log2e = 1.44269504088896338700e+00
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    n = rint(x * log2e)
    r = fma(-n, ln2_lo, fma(-n, ln2_hi, x))
    p = fma(r, 1.6059043836821613e-10, 2.08767569878681e-09)
    for k in (2.505210838544172e-08, 2.755731922398589e-07, 2.7557319223985893e-06,
              2.48015873015873e-05, 1.984126984126984e-04, 1.388888888888889e-03,
              8.333333333333333e-03, 4.1666666666666664e-02, 1.6666666666666666e-01, 0.5, 1.0, 1.0):
        p = fma(r, p, k)
    e = ldexp(p, int(fmax(fmin(n, 2000.0), -2000.0)))
    return 0.0 if x < -746.0 else (INF if x > 710.0 else e)


K_INV_LN2N = float.fromhex("0x1.71547652b82fep+6")
K_NEG_LN2_HI_N = float.fromhex("-0x1.62e42ff000000p-7")
K_NEG_LN2_LO_N = float.fromhex("0x1.718432a1b0e26p-41")
K_SHIFT = float.fromhex("0x1.8p52")


def exp_tab(x, tab, nonpos=False):
    """tab: exp_table().  k is taken the device's way: the low word of kdm, as a signed int."""
    kdm = fma(x, K_INV_LN2N, K_SHIFT)
    kd = kdm - K_SHIFT
    r = fma(kd, K_NEG_LN2_LO_N, fma(kd, K_NEG_LN2_HI_N, x))
    ki = low_word_int(kdm)
    tx, ty = tab[ki & 63]
    r2 = r * r
    c45 = fma(r, 1.0 / 120.0, 1.0 / 24.0)
    c23 = fma(r, 1.0 / 6.0, 0.5)
    p = fma(r2, fma(r2, c45, c23), r)
    v = tx + fma(tx, p, ty)
    e = ldexp(v, ki >> 6)
    if nonpos:
        return 0.0 if x < -746.0 else e
    return 0.0 if x < -746.0 else (INF if x > 710.0 else e)


def exp_nhalf(y, tab, nonpos=False):
    """exp(-y/2) on doubled intermediates; tab: exp_table() (t.x is halved here, as the
    kernel halves it when it stages the table)."""
    kdm = fma(y, -0.5 * K_INV_LN2N, K_SHIFT)
    kd = kdm - K_SHIFT
    r = fma(kd, 2.0 * K_NEG_LN2_LO_N, fma(kd, 2.0 * K_NEG_LN2_HI_N, -y))
    ki = low_word_int(kdm)
    tx, ty = tab[ki & 63]
    tx = tx * 0.5
    r2 = r * r
    c45 = fma(r, (1.0 / 120.0) / 16.0, (1.0 / 24.0) / 8.0)
    c23 = fma(r, (1.0 / 6.0) / 4.0, 0.25)
    p = fma(r2, fma(r2, c45, c23), r)
    v = fma(tx, 2.0, fma(tx, p, ty))
    e = ldexp(v, ki >> 6)
    if nonpos:
        return 0.0 if y > 1492.0 else e
    return 0.0 if y > 1492.0 else (INF if y < -1420.0 else e)


# ------------------------------------------------------------- device RNG
def rng_sincos2pi(word):
    """rng_sincos2pi of u = (word + 1) 2^-32, the uniform bm_pair forms."""
    u = (float(word) + 1.0) * 2.0 ** -32
    x = 4.0 * u
    n = rint(x)
    r = x - n
    t = r * 1.57079632679489661923
    return _quadrant(n, ksin0(t), kcos(t, 0.0))


def rng_sincos2pi_tab(word, T):
    B = (word + 1) & 0xFFFFFFFF
    ts, tc = T.sc[B >> 24]
    r = float(B & 0xFFFFFF) * float.fromhex("0x1.921fb54442d18p-30")
    z = r * r
    ps = fma(z, fma(z, fma(z, 1.0 / 362880.0, -1.0 / 5040.0), 1.0 / 120.0), -1.0 / 6.0)
    sr = fma(r * z, ps, r)
    pc = fma(z, fma(z, fma(z, 1.0 / 40320.0, -1.0 / 720.0), 1.0 / 24.0), -0.5)
    cr = fma(z, pc, 1.0)
    return fma(ts, cr, tc * sr), fma(tc, cr, -(ts * sr))


def rng_log_tab(word, T):
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    d = float(word) + 1.0
    m, e = math.frexp(d)
    e -= 32
    if m < 0.70710678118654752440:
        m = m + m
        e -= 1
    hi = (bits(m) >> 32) & 0xFFFFFFFF
    j = ((hi >> 13) & 0x7F) | (((hi >> 20) & 1) << 7)
    invc, lhi = T.li[j]
    r = fma(m, invc, -1.0)
    z = r * r
    q = fma(r, -1.0 / 8.0, 1.0 / 7.0)
    for k in (-1.0 / 6.0, 1.0 / 5.0, -1.0 / 4.0, 1.0 / 3.0, -0.5):
        q = fma(r, q, k)
    de = float(e)
    return fma(de, ln2_hi, lhi) + (r + (fma(de, ln2_lo, T.ll[j]) + z * q))


# ----------------------------------------------------------- evaluation
def evaluate(name, args):
    """The restatement `name` over the rows of args (n x 4, as slam_debug_math
    takes them): n x 2 results, unused results 0."""
    tab = exp_table() if name.startswith("exp_") else None
    T = RngTabs() if name in ("heading_sincos_tab", "rng_log_tab", "rng_sincos2pi_tab") else None
    out = np.zeros((len(args), 2))
    for i, row in enumerate(args):
        a = float(row[0])
        if name == "fast_sincos":
            out[i] = fast_sincos(a)
        elif name == "small_sincos":
            out[i] = small_sincos(a)
        elif name == "rotate_sc":
            out[i] = rotate_sc(*(float(v) for v in row))
        elif name == "heading_sincos_tab":
            out[i] = heading_sincos_tab(a, T)
        elif name == "exp_lean":
            out[i, 0] = exp_lean(a)
        elif name in ("exp_tab", "exp_tab_nonpos"):
            out[i, 0] = exp_tab(a, tab, name.endswith("nonpos"))
        elif name in ("exp_nhalf", "exp_nhalf_nonpos"):
            out[i, 0] = exp_nhalf(a, tab, name.endswith("nonpos"))
        elif name == "rng_log_tab":
            out[i, 0] = rng_log_tab(int(a), T)
        elif name == "rng_sincos2pi_tab":
            out[i] = rng_sincos2pi_tab(int(a), T)
        elif name == "rng_sincos2pi":
            out[i] = rng_sincos2pi(int(a))
        else:
            raise KeyError(name)
    return out


# ------------------------------------------------------- argument sets
# Each set: a seeded random part of 2,048 plus the edges at which the routine
# can go wrong.  Returned as float64 arrays (one operand) unless noted.
def _nbrs(x):
    return [np.nextafter(x, -INF), x, np.nextafter(x, INF)]


def hard_sincos_search(count=200, kmax=333772):
    """The `count` doubles below 2^19 closest to a multiple of pi/2: for k in
    [1, kmax] the doubles on both sides of k pi/2, ranked by their distance
    from it in units of their own ulp.  Needs mpmath (the generator and the
    accuracy test call it; the device test reads the fixture)."""
    import mpmath as mp
    with mp.workprec(200):
        hp = mp.pi / 2
        cand = []
        for k in range(1, kmax + 1):
            t = k * hp
            x = float(t)
            if not x < 2.0 ** 19:
                break
            d = abs(mp.mpf(x) - t)
            cand.append((float(d / math.ulp(x)), x))
    cand.sort()
    return np.array(sorted(x for _, x in cand[:count]))


def args_fast_sincos(hard):
    rs = np.random.RandomState(101)
    xs = list(rs.uniform(-8.0, 8.0, 1024)) + list(rs.uniform(-2.0 ** 19, 2.0 ** 19, 1024))
    for k in range(-40, 41):
        xs += _nbrs(k * (math.pi / 2))
    e = float(np.nextafter(2.0 ** 19, 0.0))
    xs += [e, -e, 0.0, -0.0, 5e-324, 1e-300]
    xs += list(hard)
    return np.array(xs)


def args_sincos_handoff():
    return np.array([2.0 ** 19, -2.0 ** 19, float(np.nextafter(2.0 ** 19, INF)), 1e6, -1e10, 1e22,
                     INF, -INF, NAN])


def args_small_sincos():
    rs = np.random.RandomState(102)
    sg = lambda n: np.where(rs.randint(0, 2, n) == 1, 1.0, -1.0)     # noqa: E731
    xs = list(rs.uniform(-0.0625, 0.0625, 683))
    xs += list(sg(683) * rs.uniform(0.0625, K_PIO4, 683))
    xs += list(sg(682) * rs.uniform(K_PIO4, 8.0, 682))
    for v in (0.0625, -0.0625, K_PIO4, -K_PIO4):
        xs += _nbrs(v)
    xs += [0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, 1e-300]
    return np.array(xs)


def args_rotate_sc():
    rs = np.random.RandomState(103)
    a = rs.uniform(-math.pi, math.pi, 2048)
    d = np.concatenate([rs.uniform(-1.0 / 16, 1.0 / 16, 1024), rs.uniform(-math.pi, math.pi, 1024)])
    return np.stack([np.sin(a), np.cos(a), np.sin(d), np.cos(d)], axis=1)


def args_heading_sincos_tab():
    rs = np.random.RandomState(104)
    xs = list(rs.uniform(-math.pi - 0.1, math.pi + 0.1, 2048))
    for j in range(-128, 129):
        xs += [j * math.pi / 128 - 1e-12, j * math.pi / 128, j * math.pi / 128 + 1e-12]
    lim = 3.2415926535897931
    xs += [lim, -lim, float(np.nextafter(lim, INF)), -float(np.nextafter(lim, INF)), 0.0, -0.0,
           5e-324, 1e-300, -1e-17]
    return np.array(xs)


def args_exp(nonpos=False):
    """exp_lean and exp_tab<0>; nonpos: the same arguments restricted to x <= 0 (and NaN)."""
    rs = np.random.RandomState(105)
    xs = list(rs.uniform(-746.0, 710.0, 1792)) + list(rs.uniform(-1e-3, 1e-3, 256))
    for v in (-746.0, 710.0):
        xs += _nbrs(v)
    xs += [-745.2, -708.4, 709.78, 1e-3, -1e-3, 0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300]
    ln2 = math.log(2.0)
    for k in range(-47700, 45500, 997):           # k ln2/64: the table-slot edges' neighbourhood
        xs += [k * ln2 / 64, (k + 0.5) * ln2 / 64]
    for k in range(-1076, 1025, 7):               # k ln2/2: the binade edges of the result
        xs += [k * ln2 / 2, k * ln2]
    xs = [x for x in xs if -750.0 <= x <= 712.0]
    xs += [INF, -INF, NAN]
    xs = np.array(xs)
    if nonpos:
        xs = xs[~(xs > 0.0) & ~np.isposinf(xs)]
    return xs


def args_exp_nhalf(nonpos=False):
    """exp_nhalf<0>: y in [-1420, 1492]; nonpos: the y >= 0 (and NaN) of the same set."""
    rs = np.random.RandomState(106)
    ys = list(rs.uniform(-1420.0, 1492.0, 1792)) + list(rs.uniform(-2e-3, 2e-3, 256))
    for v in (-1420.0, 1492.0):
        ys += _nbrs(v)
    ys += [1490.4, 1416.8, -1419.56, 0.0, -0.0, 1491.99, 1492.5, 1e5]
    ys += [5e-324, -5e-324, 1e-310, -1e-310, 2.0 ** -1073, 2.2250738585072014e-308,
           -2.2250738585072014e-308, 3e-308]      # y / 2 subnormal
    ln2 = math.log(2.0)
    for k in range(-47700, 45500, 997):
        ys += [-2.0 * (k * ln2 / 64), -2.0 * ((k + 0.5) * ln2 / 64)]
    for k in range(-1076, 1025, 7):
        ys += [-k * ln2, -2.0 * k * ln2]
    ys = [y for y in ys if -1424.0 <= y <= 1e5]
    ys += [INF, -INF, NAN]
    ys = np.array(ys)
    if nonpos:
        ys = ys[~(ys < 0.0) & ~np.isneginf(ys)]
    return ys


_WORD_EDGES = [0, 1, 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2, 2 ** 32 - 1]


def args_rng_sincos_words():
    """32-bit words (as doubles): random, the ends, and (j << 24) + d -- the table-slot
    edges and the quarter turns."""
    rs = np.random.RandomState(107)
    w = [int(v) for v in rs.randint(0, 2 ** 32, 2048, dtype=np.uint64)] + _WORD_EDGES
    w += [((j << 24) + d) % 2 ** 32 for j in range(256) for d in (-2, -1, 0, 1)]
    return np.array(w, dtype=np.float64)


def args_rng_log_words():
    """The words above, plus d = word + 1 on both sides of every log slot edge (three
    binades), of the m < sqrt(1/2) switch in every binade and of every power of two."""
    w = [int(v) for v in args_rng_sincos_words()]
    ds = []
    for e in (8, 19, 31):
        for f in range(128):
            d0 = (2 ** e) + f * 2 ** (e - 7)
            ds += [d0 - 1, d0, d0 + 1]
    for e in range(0, 32):
        d0 = int(math.floor(math.sqrt(2.0) * 2.0 ** e))
        ds += [d0 - 1, d0, d0 + 1, d0 + 2]
    for e in range(0, 33):
        ds += [2 ** e - 1, 2 ** e, 2 ** e + 1]
    w += [d - 1 for d in ds if 1 <= d <= 2 ** 32]
    return np.array(w, dtype=np.float64)


def args_sqrt_pos():
    rs = np.random.RandomState(108)
    xs = [0.0, 2.0 ** -1022, np.finfo(np.float64).max] + _nbrs(1.0)
    for k in list(range(2, 200)) + [2 ** 26 + 1, 94906265, 3 ** 20]:
        xs += _nbrs(float(k) * float(k))
    xs += [2.0 ** e for e in range(-1022, 1024, 3)]               # powers of 2 and of 4
    xs += list(np.ldexp(rs.uniform(1.0, 2.0, 2048), rs.randint(-1022, 1024, 2048)))
    xs += list(rs.uniform(0.0, 45.0, 1024))                       # the RNG's -2 log u
    return np.array(xs)


def pad4(a):
    """Operands as slam_debug_math takes them: n x 4."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a[:, None]
    out = np.zeros((a.shape[0], 4))
    out[:, :a.shape[1]] = a
    return out


def same_bits(a, b):
    """Elementwise: equal 64-bit patterns, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def dd(hi, lo):
    """The double-double (hi, lo) as a rational."""
    return Fraction(float(hi)) + Fraction(float(lo))


def ulp_err(got, hi, lo, floor=0.0):
    """|got - (hi + lo)| in ulp of max(|hi|, floor)."""
    return float(abs(Fraction(float(got)) - dd(hi, lo)) / Fraction(math.ulp(max(abs(float(hi)), floor))))
