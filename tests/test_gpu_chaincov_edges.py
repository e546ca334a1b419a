"""The covariance kernels (kernels_chaincov.hip) at the edges of their k loop and of their tiles, with the checks and bounds of
tests/test_gpu_chaincov.py::test_matrix_and_trace_against_longdouble:
  K = 4 | 5      the groups of four k of one MFMA;
  K = 16 | 17    the split of a 64-chunk over the four wavefronts (k0 = 16 wv + 4 q): one wavefront busy | a second one;
  K = 63 | 64    one chunk with a dead k | full, the prefetch guard kb + KC < K false at its edge;
  K = 128 | 129  two chunks, the guard false for the second | a third chunk of one k;
  n = 1, 2, 31   fewer rows than one 32 x 32 tile; n = 32 | 33: one tile | three; n = 81: three tiles a side, the last one cut;
and one negative control: a changed last entry Y[n - 1, K - 1] moves C[n - 1, n - 1] and the error out of their bounds."""
import numpy as np
import pytest

import test_gpu_chaincov as CC
from test_gpu_chaincov import EPS, cov_longdouble, dev, elementwise_bound, fro, make_steps, random_spd

pytestmark = pytest.mark.gpu
NS = [1, 2, 31, 32, 33, 81]
KS = [2, 4, 5, 16, 17, 63, 64, 128, 129]
TILE, KGROUP, KWAVE, KCHUNK = 32, 4, 16, 64
assert {TILE - 1, TILE, TILE + 1} <= set(NS) and min(NS) == 1
assert all({e, e + 1} <= set(KS) for e in (KGROUP, KWAVE, 2 * KCHUNK)) and {KCHUNK - 1, KCHUNK} <= set(KS)


@pytest.mark.parametrize("offset", [0.0, 50.0])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", NS)
def test_matrix_and_trace_at_the_edges(n, K, offset):
    CC.test_matrix_and_trace_against_longdouble(n, K, 3, offset)


@pytest.mark.parametrize("n,K", [(33, 129), (32, 17)])
def test_changed_last_entry_leaves_the_bounds(n, K):
    """the last entry moved by 64 of its row's scale away from the row mean: the last diagonal entry of the matrix and the error,
    compared with the references and bounds of the unchanged step"""
    from parmgmc_amd import ChainCov

    (Y,) = make_steps(n, K, 1, 50.0, seed=n + 7 * K)
    Sigma = random_spd(n, seed=n + K)
    sn = fro(Sigma)
    Cref, m = cov_longdouble(Y)
    E = elementwise_bound(Y, m)
    err_ref = fro(Cref - Sigma) / sn
    bound = float(fro(E) / sn + n * n * EPS * err_ref)
    Y2 = Y.copy()
    spread = float(np.abs(Y[n - 1] - float(m[n - 1])).max())
    Y2[n - 1, K - 1] += 64 * spread if Y[n - 1, K - 1] >= float(m[n - 1]) else -64 * spread
    Cnew, _ = cov_longdouble(Y2)
    assert abs(Cnew[-1, -1] - Cref[-1, -1]) >= 100 * E[-1, -1] and abs(fro(Cnew - Sigma) / sn - err_ref) >= 100 * bound  # the references move
    got = {}
    for name, arr in (("unchanged", Y), ("changed", Y2)):
        cc = ChainCov.from_dense(Sigma, K, max_steps=1)
        Yd = dev(arr)
        cc.update(Yd)
        got[name] = cc.covariance(Yd).cpu().numpy(), cc.errors()[0]
    C0, e0 = got["unchanged"]
    C1, e1 = got["changed"]
    assert (np.abs(C0 - Cref) <= E).all() and abs(e0 - err_ref) <= bound
    print(f"n={n} K={K}: C[n-1, n-1] off by {float(abs(C1[-1, -1] - Cref[-1, -1]) / E[-1, -1]):.3e} bounds, the error by {float(abs(e1 - err_ref)) / bound:.3e} bounds")
    assert abs(C1[-1, -1] - Cref[-1, -1]) > E[-1, -1] and abs(e1 - err_ref) > bound
    assert np.array_equal(C1[:-1, :-1], C0[:-1, :-1])  # the other rows' entries keep their bits
