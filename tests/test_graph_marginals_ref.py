"""The host reference of the marginal-covariance tests against mpmath.

tests/graph_marginals_ref.py refines NumPy's inverse with extended-precision
residuals; here its result is checked against an inverse computed at 50
decimal digits on the reference's own H matrices (tests/golden/graph.npz), so
the GPU tests' bars rest on a reference whose error is known.
"""
import mpmath
import numpy as np
import pytest

from conftest import golden
from graph_marginals_ref import gate, ref_columns


@pytest.mark.parametrize("k", [3, 50])
def test_refined_columns_match_mpmath(k):
    H = golden("graph")[f"demo{k}_H"]
    n = H.shape[0]
    assert n == {3: 9, 50: 57}[k]
    X64, Xref, spread = ref_columns(H, np.arange(n))
    with mpmath.workdps(50):
        Xmp = mpmath.matrix(H.tolist()) ** -1
        exact = np.array([[float(Xmp[i, j]) for j in range(n)] for i in range(n)])
    bound = 4 * np.spacing(np.abs(exact).max())
    print(f"demo{k}: max|Xref - exact| = {np.abs(Xref - exact).max():.3g}, bound {bound:.3g}, "
          f"spread {spread:.3g}")
    assert np.abs(Xref - exact).max() <= bound
    assert spread == np.abs(Xref - X64).max()
    np.testing.assert_array_equal(X64, np.linalg.inv(H))


def test_singular_demo_iteration_is_not_calculable():
    g = golden("graph")
    H = g["demo20_H"]
    assert np.linalg.eigvalsh(0.5 * (H + H.T))[0] < 0        # the reference's singular branch
    assert g["demo20_stats"][0] == 0.0
    assert not gate(H)
    assert gate(g["demo3_H"]) and gate(g["demo50_H"])
