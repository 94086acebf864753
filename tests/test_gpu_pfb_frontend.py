"""The drop-in's ParticleFilterEnsemble (particle_filter.py) on the GPU: filter b
of the ensemble is the drop-in ParticleFilter run alone from np.random.seed(seed
+ b) -- the same draws in the same order, the same kernels' arithmetic -- so
main_pf's outputs agree bit for bit (host noise, product likelihood)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("motion", ["linear", "velocity"])
def test_ensemble_member_is_the_drop_in_filter(motion):
    import particle_filter as pfm
    B, n, steps, seed = 3, 300, 14, 5
    rs = np.random.RandomState(2)
    lms = rs.uniform(-10, 10, (B, 6, 2))
    ens = pfm.ParticleFilterEnsemble(100, B, n_particles=n, landmarks=lms, motion=motion, seed=seed)
    got = [ens.main_pf() for _ in range(steps)]
    ens.close()
    assert got[0][1].shape == (B, 3, 1) and got[0][2].shape == (B, 3, 1)
    assert got[0][3].shape == (B, 3, n) and got[0][5].shape == (B,) and got[0][6].shape == (B,)
    n_res = 0
    for b in range(B):
        np.random.seed(seed + b)
        one = pfm.ParticleFilter(100, n_particles=n, landmarks=lms[b], motion=motion)
        for k in range(steps):
            lm, x_true, x_est, px, q, idx, val = one.main_pf()
            n_res += one.dev.last["resampled"]
            g = got[k]
            np.testing.assert_array_equal(g[0][b], lm)
            np.testing.assert_array_equal(g[1][b], x_true)
            np.testing.assert_array_equal(g[2][b], x_est)
            np.testing.assert_array_equal(g[3][b], px)
            assert g[5][b] == idx and g[6][b] == val, (b, k)
        one.dev.close()
    assert n_res >= 1                                     # the comparison went through resampling steps
