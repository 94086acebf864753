"""Host restatement of fastmath.hpp's exp_tab (the product likelihood's exp):
the header's 64-entry table, k = round(x 64/ln2) by the 1.5 2^52 shift,
Cody-Waite reduction, degree-5 polynomial, every fma emulated exactly
(Fraction arithmetic, one rounding).  Pins the header's accuracy claim:
under 0.9 ulp against mpmath's correctly rounded exp on arguments the
likelihood produces (x = -q/2 <= 0, normal results)."""
import math
import random

import pytest

from fastmath_ref import exp_nhalf, exp_tab          # the restatements, operation by operation
from fastmath_ref import exp_table as _table

mp = pytest.importorskip("mpmath")


def test_exp_tab_under_0p9_ulp():
    tab = _table()
    mp.mp.dps = 40
    rng = random.Random(7)
    xs = [-rng.uniform(0.0, 700.0) for _ in range(1500)] + [-rng.uniform(0.0, 1e-3) for _ in range(200)]
    worst = 0.0
    for x in xs:
        got = exp_tab(x, tab)
        ref = mp.exp(mp.mpf(x))
        ulp = math.ulp(float(ref))
        worst = max(worst, abs(float((mp.mpf(got) - ref) / ulp)))
    assert worst < 0.9, worst


def test_exp_nhalf_bits_equal_exp_tab():
    """The product factor's exp(-q/2) without forming q/2 gives exp_tab(-q/2)'s bits
    (q >= 0 in the likelihood; also the rho path's 2|a|, tiny and subnormal q, the range edges)."""
    tab = _table()
    rng = random.Random(11)
    ys = [rng.uniform(0.0, 1500.0) for _ in range(1500)] + [rng.uniform(0.0, 1e-3) for _ in range(300)]
    ys += [math.ldexp(rng.uniform(1.0, 2.0), -rng.randrange(20, 1074)) for _ in range(300)]
    ys += [0.0, 5e-324, 2.2250738585072014e-308, 1490.0, 1491.99, 1492.0, 1492.5, 1e5]
    ys += [2.0 * rng.uniform(0.0, 700.0) for _ in range(300)]
    for y in ys:
        x = -y * 0.5
        want = exp_tab(x, tab)
        got = exp_nhalf(y, tab)
        assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (y, got, want)
