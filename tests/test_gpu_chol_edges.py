"""The dense Cholesky coarse sampler (pmg_chol.c + kernels_dense.hip: 32x32-tile right-looking factorisation with the
panel formed from the inverse diagonal tile, MFMA trailing updates, the blocked inverse W = L^-1 by recursive doubling,
two triangular products per sample) against high-precision references at its tile edges and at bench size.

Bounds (chol_edge_refs.py, fixed before the first device run; u = 2^-53, kappa = kappa_2(A), c = C_FWD = 8):
  factor  ||A - L L^T||_F / ||A||_F <= gamma_{n+1} trace(A) / ||A||_F, L lower triangular with a positive diagonal
  solve   ||x - A^-1 b||_inf / ||A^-1 b||_inf <= c n kappa u   (reference: LU + 2 long-double refinement steps)
  sample  ||y - y*||_inf / ||y*||_inf <= c n kappa u   (y*: mpmath at 40 digits for n <= 97, else the oracle's L^-T (L^-1 b + xi))
  noise   ||L_dev^T (y - x) - xi||_2 / ||xi||_2 <= c n sqrt(kappa) u
  xi      the noise the sample drew (same kernel, read through vec_set_random_standard_normal) is the oracle's noise_rows
          stream to XI_TOL; y* and the noise check use the drawn xi, so that they measure the sampler's arithmetic only
Largest measured error as a fraction of its bound, on an MI355X (factor / solve / sample / noise / xi):
  tile-edge sweep, n = 1 .. 1025, kappa 10 .. 1e10       0.20 / 0.012 / 0.018 / 0.037 / 0.0052
  bench size, n = 4913 (Galerkin, device coarsest, LRC)   6.2e-5 / 1.5e-5 / 3.0e-5 / 2.3e-5 / 0.0048
  failing minors, recovery after each failure            1.7e-3 / 7.6e-5 / 1.2e-4 / 3.5e-4 / 0.0052
(the module prints these at its end).  The explicit-inverse panel stays inside the classical bound everywhere.
Each family also runs a negative control that must fail its check: one entry of a far-off-diagonal tile of L 1e-8 off
(factor), the reference noise one counter on (sample), a 1e-8 change in the strictly lower triangle (bit equality)."""
import numpy as np
import pytest
import scipy.sparse as sp

import oracle as O
from chol_edge_refs import (
    dense_spd,
    eig_range,
    factor_bound,
    factor_error,
    fwd_bound,
    lapack_info,
    lowrank_sum,
    noise_bound,
    noise_error,
    rel_inf,
    sample_ref,
    solve_ref,
    to_csr,
    with_failing_minor,
)
from test_lrc import observation_matrix

pytestmark = pytest.mark.gpu

EDGE_N = [1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 255, 256, 257, 1023, 1024, 1025]
KAPPAS = [10.0, 1e6, 1e10]
SEED, COUNTER = 0x5EED, 41
XI_TOL = 1e-13  # device noise vs the oracle's noise_rows, relative in the inf-norm
WORST: dict = {}  # family -> largest error / bound per check, printed at the end of the module


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def record(family, check, err, bound):
    w = WORST.setdefault(family, {})
    w[check] = max(w.get(check, 0.0), err / bound)
    assert err <= bound, (family, check, err, bound)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for fam, w in WORST.items():
        print(f"chol edges {fam}: " + ", ".join(f"{k} {v:.3g}" for k, v in w.items()))


def device_run(ch, b, seed=SEED, counter=COUNTER):
    """(L, x, y, xi): the factor, the deterministic solve and the noisy sample for b, and the noise the sample drew"""
    import torch

    from parmgmc_amd import vec_set_random_standard_normal

    bd = dev(b)
    x = torch.zeros_like(bd)
    y = torch.zeros_like(bd)
    xi = torch.zeros_like(bd)
    ch.sample(bd, x, 0, 0, noisy=False)
    ch.sample(bd, y, seed, counter, noisy=True)
    vec_set_random_standard_normal(xi, seed, counter)  # the same fill_normal_rows stream pmg_chol_sample draws
    torch.cuda.synchronize()
    return ch.factor(), x.cpu().numpy(), y.cpu().numpy(), xi.cpu().numpy()


def check_sampler(family, A, ch, rng, L_ref=None, full=True):
    """factor, solve, sample and noise checks of the sampler ch of A (dense float64, the exact entries the device
    factors); returns (L, b, y, y*, kappa) for negative controls"""
    n = A.shape[0]
    lo, hi = eig_range(A)
    kappa = hi / lo
    b = np.sqrt(lo) * rng.standard_normal(n)
    L, x, y, xi = device_run(ch, b)
    assert np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0)
    record(family, "factor", factor_error(A, L), factor_bound(A))
    record(family, "solve", rel_inf(x, solve_ref(A, b)), fwd_bound(n, kappa))
    # the references take the device's own noise: its Box-Muller rounds log/sin/cos differently from the oracle's libm in
    # the last bits, which at n = 1 (y = b + xi) is larger than c n kappa u.  The stream itself is the oracle's:
    record(family, "xi", rel_inf(xi, O.noise_rows(n, SEED, COUNTER)), XI_TOL)
    if full:
        ys = sample_ref(A, b, xi, L_ref)
        record(family, "sample", rel_inf(y, ys), fwd_bound(n, kappa))
    else:
        ys = None
    record(family, "noise", noise_error(L, y - x, xi), noise_bound(n, kappa))
    return L, b, y, ys, kappa


# ------------------------------------------------------------------------------------------------------------------
# (a) tile edges: 1, 2, 3, 8, 9, 32 and 33 tiles, dense SPD matrices (data in every MFMA and inverse tile)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("n", EDGE_N)
def test_tile_edges_dense(n, kappa):
    from parmgmc_amd import CholSampler

    A = dense_spd(n, kappa, 1000 + n)
    ch = CholSampler(*to_csr(A))
    L, b, y, ys, kap = check_sampler("edges", A, ch, np.random.default_rng(n))
    if n == 257 and kappa == 1e6:  # negative controls
        i0 = n - n % 32
        blk = np.abs(L[i0:, :32])
        i, j = np.unravel_index(np.argmax(blk), blk.shape)
        Lb = L.copy()
        Lb[i0 + i, j] *= 1 + 1e-8
        assert factor_error(A, Lb) > factor_bound(A)
        assert rel_inf(y, sample_ref(A, b, O.noise_rows(n, SEED, COUNTER + 1))) > fwd_bound(n, kap)


# ------------------------------------------------------------------------------------------------------------------
# (b) bench size: the 17^3 = 4913-row 27-point Galerkin operator, the device's own coarsest level, its MATLRC forms
# ------------------------------------------------------------------------------------------------------------------
_GAL = {}


def galerkin17(kappa):
    if kappa not in _GAL:
        _GAL[kappa] = O.galerkin(O.shifted_laplace(33, 33, 33, kappa).scipy(), O.q1_interp(17, 17, 17))
    return _GAL[kappa]


def _bench_check(family, A, ch, seed):
    check_sampler(family, A, ch, np.random.default_rng(seed), L_ref=np.linalg.cholesky(A))


@pytest.mark.parametrize("kappa", [10.0, 0.5])
def test_bench_size_galerkin(kappa):
    from parmgmc_amd import CholSampler

    G = galerkin17(kappa)
    assert G.shape == (4913, 4913)
    _bench_check("bench", G.toarray(), CholSampler(*to_csr(G)), 1)


def test_bench_size_device_coarsest():
    import torch

    from parmgmc_amd import MGMC, CholSampler

    mg = MGMC(257, 257, 257, 10.0, 5, keep_host=True).setup()
    rp, ci, v = mg.level_matrix(0, "A")
    mg.destroy()
    torch.cuda.synchronize()
    assert len(rp) - 1 == 4913
    A = sp.csr_matrix((v, ci, rp), shape=(4913, 4913)).toarray()
    _bench_check("bench", A, CholSampler(rp, ci, v), 2)


@pytest.mark.parametrize("k", [3, 64])
def test_bench_size_lowrank_posterior(k):
    """P = A + B S B^T with S over [1, 1e8]: precise observations, an ill-conditioned factored matrix"""
    from parmgmc_amd import CholSampler

    G = galerkin17(10.0)
    B = observation_matrix(4913, k, 30 + k)
    S = np.geomspace(1.0, 1e8, k)
    _bench_check("bench", lowrank_sum(G.toarray(), B, S), CholSampler(*to_csr(G), B=B, S=S), 3)


# ------------------------------------------------------------------------------------------------------------------
# (c) failing minors: order, message, and a correct sampler after every failure
# ------------------------------------------------------------------------------------------------------------------
def _expect_failure(csr, m, **kw):
    from parmgmc_amd import CholSampler, PMGError

    with pytest.raises(PMGError) as e:
        CholSampler(*csr, **kw)
    assert e.value.code == 81 and f"leading minor of order {m} is not positive definite" in str(e.value), str(e.value)


def test_failing_minor_orders_dense():
    from parmgmc_amd import CholSampler

    n = 129
    A = dense_spd(n, 1e3, 7)
    L0, b, y0, _, _ = check_sampler("minor", A, CholSampler(*to_csr(A)), np.random.default_rng(7))
    csr = to_csr(A)

    def recovered():
        L, x, y, _ = device_run(CholSampler(*csr), b)
        assert np.array_equal(L.view(np.int64), L0.view(np.int64)) and np.array_equal(y.view(np.int64), y0.view(np.int64))

    for m in [1, 2, 31, 32, 33, 64, 65, 97, n]:
        Bad = with_failing_minor(A, m)
        assert lapack_info(Bad) == m
        _expect_failure(to_csr(Bad), m)
        recovered()
        Bn = A.copy()
        Bn[m - 1, m - 1] = np.nan  # reference LAPACK (dpotrf2) reports a NaN pivot like a non-positive one
        _expect_failure(to_csr(Bn), m)
        recovered()
    for r in (0, 32, 64, n - 1):  # an empty CSR row: its row of the lower triangle is zero, pivot 0 at order r + 1
        rp, ci, v = csr
        keep = np.ones(len(v), bool)
        keep[rp[r] : rp[r + 1]] = False
        rp2 = np.concatenate([rp[: r + 1], rp[r + 1 :] - (rp[r + 1] - rp[r])]).astype(np.int32)
        Z = A.copy()
        Z[r, :] = 0.0
        assert lapack_info(Z) == r + 1
        _expect_failure((rp2, ci[keep], v[keep]), r + 1)
        recovered()


def test_failing_minor_bench_size():
    from parmgmc_amd import CholSampler

    G = galerkin17(10.0)
    A = G.toarray()
    m = 4900
    Bad = with_failing_minor(A, m)
    assert lapack_info(Bad) == m
    Gb = G.copy()
    Gb[m - 1, m - 1] = Bad[m - 1, m - 1]
    assert Gb.nnz == G.nnz
    _expect_failure(to_csr(Gb), m)
    check_sampler("minor", A, CholSampler(*to_csr(G)), np.random.default_rng(9), L_ref=np.linalg.cholesky(A), full=False)


# ------------------------------------------------------------------------------------------------------------------
# (d) only the lower triangle is read (LAPACKpotrf_("L"))
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [97, 257])
def test_lower_triangle_only(n):
    from parmgmc_amd import CholSampler

    A = dense_spd(n, 1e6, 50 + n)
    rng = np.random.default_rng(n)
    R = rng.standard_normal((n, n))
    b = rng.standard_normal(n)

    def bits(M):
        L, x, y, _ = device_run(CholSampler(*to_csr(M)), b)
        return [t.view(np.int64).copy() for t in (L, x, y)]

    ref = bits(A)
    nan_up = np.triu(np.full((n, n), np.nan), 1)
    for M in (np.tril(A) + np.triu(R, 1), np.tril(A), np.tril(A) + nan_up):
        got = bits(M)
        assert all(np.array_equal(g, r) for g, r in zip(got, ref))
    # negative control: a change in the strictly lower triangle is seen
    got = bits(np.tril(A) + np.tril(R, -1) * 1e-8)
    assert not np.array_equal(got[0], ref[0]) and not np.array_equal(got[2], ref[2])


# ------------------------------------------------------------------------------------------------------------------
# (e) many chains: the coarse level's tri_gemv_chains at ragged and bench sizes equals the single-chain sampler bitwise
# ------------------------------------------------------------------------------------------------------------------
def _two_level(fine, coarse, kappa):
    Af = O.shifted_laplace(*fine, kappa).scipy()
    P = O.q1_interp(*coarse)
    Ac = O.galerkin(Af, P)

    def triple(M):
        M = M.tocsr()
        M.sort_indices()
        return M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64)

    return [triple(Ac), triple(Af)], [None, triple(P)]


@pytest.mark.parametrize("fine,coarse", [((65, 1, 1), (33, 1, 1)), ((33, 33, 33), (17, 17, 17))])
def test_chains_coarse_edges(fine, coarse):
    import torch

    from parmgmc_amd import MGMC

    ops, ps = _two_level(fine, coarse, 10.0)
    assert len(ops[0][0]) - 1 == int(np.prod(coarse))
    mg = MGMC.from_hierarchy(ops, ps)
    mg.set_coarse("cholsampler")
    mg.setup()
    n = mg.n
    rng = np.random.default_rng(int(np.prod(coarse)))
    b = dev(rng.standard_normal(n))
    seeds = [0xC0FFEE + 131 * c for c in range(65)]
    for nchains in (1, 9, 65):
        for guesszero in (False, True):
            Y0 = dev(rng.standard_normal((n, nchains)))
            Y = Y0.clone()
            assert mg.sample_chains(b, Y, 2, seeds[:nchains], counter0=5, guesszero=guesszero) == 7
            for c in range(nchains):
                y = Y0[:, c].contiguous()
                mg.sample(b, y, 2, seeds[c], counter0=5, guesszero=guesszero)
                assert torch.equal(Y[:, c].view(torch.int64), y.view(torch.int64)), (nchains, guesszero, c)
