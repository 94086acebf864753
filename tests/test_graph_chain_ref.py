"""The NumPy restatement of the chain preconditioner (tests/graph_chain_ref.py,
DESIGN 8.5) against NumPy's own dense algebra, and the CPU iteration table of
DESIGN 8.5.  No GPU.

apply against np.linalg.solve on the explicitly built M: the bar is the one
test_gpu_graph_chain.py holds the device to, cond(M) * 1e-12 * max|z| (a
backward-stable solve of a system with that condition number).

The table (PCG, tol 1e-10, the graph recipe of graph_chain_ref.table_system):

   T  odometry  block-Jacobi  S=2  S=4  S=16  S=64  whole chain
  72  no                  75   63   60    57    55           55
  72  yes                196  145  110    43    25           19
 300  no                  89   83   80    78    78           77
 300  yes                403  278  195    89    50           21

Those counts came from a PCG with another summation order; a difference of one
or two is expected (DESIGN 8.5 lists the counts found here beside them), so the
rows are held to +-2.
"""
import numpy as np
import pytest

import graph_chain_ref as cr

TABLE = {(72, False): (75, 63, 60, 57, 55, 55), (72, True): (196, 145, 110, 43, 25, 19),
         (300, False): (89, 83, 80, 78, 78, 77), (300, True): (403, 278, 195, 89, 50, 21)}
COLUMNS = (0, 2, 4, 16, 64, 1 << 20)          # 0: block-Jacobi; the last: the whole chain


@pytest.mark.parametrize("name", cr.CASES)
def test_apply_is_the_solve_with_m(name):
    H, b = cr.case_system(name)
    nt = len(b) // 3
    bsr = cr.bsr_from_dense(H)
    rs = np.random.RandomState(17)
    vecs = (-b, rs.standard_normal(3 * nt))
    for S in (1, 2, 4, 64):
        M = cr.build_m(*bsr, nt, S)
        # symmetric by construction outside the diagonal blocks, to rounding inside them
        np.testing.assert_allclose(M, M.T, rtol=0, atol=1e-15 * np.abs(M).max())
        lam = np.linalg.eigvalsh(0.5 * (M + M.T))
        assert lam[0] > 0.0, (name, S, lam[0])
        Sinv, G, used, bad = cr.factor(*bsr, nt, S)
        assert bad == 0
        # the blocks used: every (r, r+1) slot that does not cross a segment boundary
        rows, cols, _ = bsr
        want = int(np.sum((cols == rows + 1) & (rows // S == cols // S)))
        assert used == want and (used == 0) == (S == 1)
        cond = lam[-1] / lam[0]
        for r in vecs:
            z = cr.apply(Sinv, G, S, r)
            ref = np.linalg.solve(M, r)
            gap = np.abs(z - ref).max()
            assert gap <= cond * 1e-12 * np.abs(ref).max(), (name, S, gap, cond)


def test_gaps_case_has_no_slot_at_the_gaps():
    H, _ = cr.case_system("gaps")
    for a, b in cr.GAPS:
        assert not H[3 * a:3 * a + 3, 3 * b:3 * b + 3].any()
    H, _ = cr.case_system("mixed200")
    for a, b in cr.GAPS:
        assert H[3 * a:3 * a + 3, 3 * b:3 * b + 3].any()


def test_segment_one_is_block_jacobi():
    H, b = cr.case_system("mixed72")
    nt = len(b) // 3
    Sinv, G, used, _ = cr.factor(*cr.bsr_from_dense(H), nt, 1)
    assert used == 0 and not G.any()
    for r in range(nt):
        np.testing.assert_array_equal(Sinv[r], np.linalg.inv(H[3 * r:3 * r + 3, 3 * r:3 * r + 3]))


def test_bad_pivots_are_counted():
    H, b = cr.case_system("odom65")
    nt = len(b) // 3
    rows, cols, vals = cr.bsr_from_dense(H)
    d = int(np.flatnonzero((rows == 7) & (cols == 7))[0])
    for value in (np.nan, np.inf):
        v = vals.copy()
        v[d, 1, 1] = value
        with np.errstate(all="ignore"):
            assert cr.factor(rows, cols, v, nt, 1)[3] == 1
            assert cr.factor(rows, cols, v, nt, 64)[3] >= 1
    v = vals.copy()
    v[d] = -v[d]                                  # a negative definite diagonal block
    assert cr.factor(rows, cols, v, nt, 1)[3] == 1
    # and the PCG ends as "not positive definite" on a preconditioner that is not
    Sinv, G, _, _ = cr.factor(rows, cols, v, nt, 1)
    Hbad = cr.dense_from_bsr(rows, cols, v, nt)
    assert cr.pcg(Hbad, b, lambda r: cr.apply(Sinv, G, 1, r), max_iter=500)[2] == 2


@pytest.mark.parametrize("T,with_odom", sorted(TABLE))
def test_iteration_table(T, with_odom):
    got = tuple(cr.table_iterations(T, with_odom, S) for S in COLUMNS)
    print(f"T = {T}, odometry {'yes' if with_odom else 'no'}: PCG iterations {got} "
          f"(DESIGN 8.5's CPU table: {TABLE[T, with_odom]})")
    # the counts fall with S
    assert all(a >= b for a, b in zip(got, got[1:])), got
    if with_odom:
        assert all(a > b for a, b in zip(got, got[1:])), got
    for g, t in zip(got, TABLE[T, with_odom]):
        assert abs(g - t) <= 2, (got, TABLE[T, with_odom])
    if with_odom:
        # S = 64 against block-Jacobi: the table's ratios are 7.8 and 8.1
        assert 4 * got[4] <= got[0], got
        # ... and the off-diagonal blocks are what buys it: without them (S = 1) it fails
        assert 4 * cr.table_iterations(T, True, 1) > got[0]


def test_pcg_solves_the_system():
    H, b = cr.table_system(72, True)
    nt = len(b) // 3
    ref = -np.linalg.solve(H, b)
    cond = np.linalg.cond(H)
    for S in (1, 64):
        x, _, status = cr.pcg(H, b, cr.chain_precond(cr.bsr_from_dense(H), nt, S), 1e-12)
        assert status == 1
        assert np.abs(x - ref).max() <= cond * 1e-12 * np.abs(ref).max()
