"""Covariance error over the chains on the device (pmg_chaincov_*): the matrix and the error trace against extended-precision
numpy with bounds computed from the inputs, agreement with the host function pmg_estimate_covariance_errors, the reference
formed from a Cholesky handle against numpy's inverse, bit-for-bit determinism, and the ex6-shaped runs driven through the
samplers' cov= keyword at every sample index."""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
ARG_OUTOFRANGE = 63


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def make_steps(n, C, T, offset, seed):
    """T steps of (n, C): unit-scale noise times a per-row scale in [0.1, 3], plus an offset (as tests/test_gpu_chainstats.py)"""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.1, 3.0, size=(n, 1))
    return [rng.standard_normal((n, C)) * scale + offset for _ in range(T)]


def random_spd(n, seed):
    rng = np.random.default_rng(seed + 1234)
    M = rng.standard_normal((n, n))
    S = M @ M.T / n + np.eye(n)
    return (S + S.T) / 2


def cov_longdouble(Y):
    """(centred covariance over the columns, row means) in np.longdouble; the lower block rows only, mirrored"""
    Yl = Y.astype(np.longdouble)
    n, C = Yl.shape
    m = Yl.sum(axis=1) / C
    Yc = Yl - m[:, None]
    out = np.empty((n, n), np.longdouble)
    for i0 in range(0, n, 256):
        i1 = min(i0 + 256, n)
        blk = Yc[i0:i1] @ Yc[:i1].T
        out[i0:i1, :i1] = blk
        out[:i1, i0:i1] = blk.T
    return out / (C - 1), m


def elementwise_bound(Y, m):
    """E_rs = (2C + 16) EPS (a a^T)_rs / (C - 1), a_r = max_c |Y_rc| + |m_r|: the worst case of a length-C fma chain plus the
    rounding of the mean, from the inputs alone"""
    C = Y.shape[1]
    a = np.abs(Y).max(axis=1) + np.abs(m.astype(np.float64))
    return (2 * C + 16) * EPS * np.outer(a, a) / (C - 1)


def fro(M):
    return np.sqrt((M.astype(np.longdouble) ** 2).sum())


CASES = [(n, C, T, offset) for n in (81, 100, 1000, 1024, 1025) for C in (2, 3, 32, 65, 1000) for T, offset in ((5 if n * C < 500000 else 3, 0.0), (3, 50.0))]


@pytest.mark.parametrize("n,C,T,offset", CASES)
def test_matrix_and_trace_against_longdouble(n, C, T, offset):
    """|C_dev - C_ref|_rs <= E_rs elementwise; |err - err_ref| <= ||E||_F / ||Sigma||_F + n^2 EPS err_ref (the second term: the
    worst case of any summation order over n^2 terms); covariance() exactly symmetric; the trace and covariance() followed by a
    longdouble norm agree within the same bound"""
    from parmgmc_amd import ChainCov

    steps = make_steps(n, C, T, offset, seed=n + 7 * C + T)
    Sigma = random_spd(n, seed=n + C)
    cc = ChainCov.from_dense(Sigma, C, max_steps=T)
    mats = []
    for Y in steps:
        Yd = dev(Y)
        cc.update(Yd)
        mats.append(cc.covariance(Yd).cpu().numpy())
    assert cc.count() == T
    errs = cc.errors()
    assert errs.shape == (T,)
    assert np.array_equal(cc.reference(), Sigma)
    sn = fro(Sigma)
    worst_el = worst_tr = worst_mt = 0.0
    for t, Y in enumerate(steps):
        Cref, m = cov_longdouble(Y)
        E = elementwise_bound(Y, m)
        Cd = mats[t]
        assert np.array_equal(Cd, Cd.T), (n, C, t)
        ratio_el = float((np.abs(Cd - Cref) / E).max())
        err_ref = fro(Cref - Sigma) / sn
        bound = float(fro(E) / sn + n * n * EPS * err_ref)
        d_tr = float(abs(errs[t] - err_ref))
        d_mt = float(abs(errs[t] - fro(Cd.astype(np.longdouble) - Sigma) / sn))
        worst_el, worst_tr, worst_mt = max(worst_el, ratio_el), max(worst_tr, d_tr / bound), max(worst_mt, d_mt / bound)
        print(f"n={n} C={C} offset={offset} step {t}: elementwise err / bound {ratio_el:.3e}; trace err {d_tr:.3e} / bound {bound:.3e}; trace vs matrix {d_mt:.3e} / bound {bound:.3e}")
        assert ratio_el <= 1.0, (n, C, t, ratio_el)
        assert d_tr <= bound, (n, C, t, d_tr, bound)
        assert d_mt <= bound, (n, C, t, d_mt, bound)
    print(f"n={n} C={C} offset={offset}: worst observed / bound: elementwise {worst_el:.3e}, trace {worst_tr:.3e}, trace vs matrix {worst_mt:.3e}")


def _csr_of_size(n):
    return {81: lambda: O.shifted_laplace(9, 9, 1, 10.0), 1024: lambda: O.ex6_matrix(32, 1e-2)}[n]()


def reference_bound(Ad):
    """8 n EPS kappa_2(A): the textbook n EPS kappa form, times 8 for the three products L, L^-1, W^T W"""
    return 8 * Ad.shape[0] * EPS * float(np.linalg.cond(Ad, 2))


def agreement_bound(Y, err_host, Sigma, Ad):
    """twice the trace bound of the test above (err_ref = the host function's value) plus the reference bound"""
    n = Y.shape[0]
    E = elementwise_bound(Y, Y.mean(axis=1))
    return 2 * float(fro(E) / fro(Sigma) + n * n * EPS * err_host) + reference_bound(Ad)


@pytest.mark.parametrize("n", [81, 1024])
@pytest.mark.parametrize("C", [3, 1000])
def test_agrees_with_the_host_function(n, C):
    """the same steps copied to the host and given to pmg_estimate_covariance_errors (ordering [sample][chain][row]), Sigma from
    create_chol on the same CSR matrix"""
    from parmgmc_amd import ChainCov, estimate_covariance_errors

    A = _csr_of_size(n)
    T = 2
    steps = make_steps(n, C, T, 50.0 if C == 3 else 0.0, seed=3 * n + C)
    cc = ChainCov.from_csr(A.rowptr, A.colidx, A.vals, C, max_steps=T)
    for Y in steps:
        cc.update(dev(Y))
    errs = cc.errors()
    S = np.concatenate([Y.T for Y in steps])
    host = estimate_covariance_errors(A.rowptr, A.colidx, A.vals, S, C)
    Ad, Sigma = A.dense(), cc.reference()
    for t in range(T):
        bound = agreement_bound(steps[t], host[t], Sigma, Ad)
        d = abs(errs[t] - host[t])
        print(f"n={n} C={C} step {t}: device {errs[t]:.15e} host {host[t]:.15e} diff {d:.3e} / bound {bound:.3e}")
        assert d <= bound, (n, C, t, d, bound)


def _three_observations(n):
    """the three-observation set-up of tests/test_gpu_lowrank_chains.py on the ex6 grid"""
    side = int(round(np.sqrt(n)))
    X, Yg = np.meshgrid(np.linspace(0, 1, side), np.linspace(0, 1, side), indexing="ij")
    pts = np.stack([X.ravel(order="F"), Yg.ravel(order="F")], 1)
    B = np.zeros((n, 3))
    for j, ctr in enumerate([(0.25, 0.3), (0.7, 0.5), (0.4, 0.8)]):
        inside = ((pts - np.asarray(ctr)) ** 2).sum(1) < 0.2**2
        B[inside, j] = 1.0 / inside.sum()
    return B, np.array([1e4, 2e4, 5e4])


@pytest.mark.parametrize("case", ["ex6", "ex1", "matlrc"])
def test_reference_from_the_cholesky_handle(case):
    """reference() of create_chol against np.linalg.inv: relative Frobenius difference <= 8 n EPS kappa_2"""
    from parmgmc_amd import ChainCov, CholSampler

    A = O.shifted_laplace(9, 9, 1, 10.0) if case == "ex1" else O.ex6_matrix(32, 1e-2)
    P = A.dense()
    lowrank = None
    if case == "matlrc":
        lowrank = _three_observations(A.n)
        P = P + lowrank[0] @ np.diag(lowrank[1]) @ lowrank[0].T
    if case == "ex1":  # through a handle that is destroyed before the reference is read
        ch = CholSampler(A.rowptr, A.colidx, A.vals)
        cc = ChainCov.from_chol(ch, 2, max_steps=1)
        ch.destroy()
    else:
        cc = ChainCov.from_csr(A.rowptr, A.colidx, A.vals, 2, max_steps=1, lowrank=lowrank)
    Sigma = cc.reference()
    assert np.array_equal(Sigma, Sigma.T)
    ref = np.linalg.inv(P)
    rel = float(fro(Sigma - ref) / fro(ref))
    bound = reference_bound(P)
    print(f"{case}: n={A.n} kappa_2={np.linalg.cond(P, 2):.3e} rel. Frobenius difference {rel:.3e} / bound {bound:.3e} = {rel / bound:.3e}")
    assert rel <= bound, (case, rel, bound)


@pytest.mark.parametrize("n,C", [(100, 3), (1024, 65), (1025, 1000)])
def test_same_bits_twice(n, C):
    """the same steps after a reset, the second time on a non-default stream: the same bits in the trace and in covariance()"""
    import torch

    from parmgmc_amd import ChainCov

    steps = [dev(Y) for Y in make_steps(n, C, 3, 50.0, seed=C)]
    cc = ChainCov.from_dense(random_spd(n, seed=C), C, max_steps=3)
    for Y in steps:
        cc.update(Y)
    e1 = cc.errors()
    m1 = cc.covariance(steps[1])
    torch.cuda.synchronize()
    cc.reset()
    assert cc.count() == 0
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for Y in steps:
            cc.update(Y)
        m2 = cc.covariance(steps[1])
    st.synchronize()
    assert np.array_equal(e1, cc.errors())
    assert torch.equal(m1, m2)
    assert np.all(np.isfinite(e1)) and np.all(e1 > 0)


def test_bookkeeping():
    """max_steps is enforced before the device is asked for anything more; windows of the trace; reset"""
    from parmgmc_amd import ChainCov
    from parmgmc_amd.capi import PMGError

    n, C = 40, 5
    steps = [dev(Y) for Y in make_steps(n, C, 2, 0.0, seed=1)]
    cc = ChainCov.from_dense(random_spd(n, 0), C, max_steps=2)
    for Y in steps:
        cc.update(Y)
    with pytest.raises(PMGError) as e:
        cc.update(steps[0])
    assert e.value.code == ARG_OUTOFRANGE
    assert cc.count() == 2
    errs = cc.errors()
    assert np.array_equal(cc.errors(1), errs[1:]) and np.array_equal(cc.errors(0, 1), errs[:1])
    with pytest.raises(PMGError):
        cc.errors(1, 2)
    cc.reset()
    cc.update(steps[1])
    assert np.array_equal(cc.errors(), errs[1:])


def _ex6_hierarchy():
    from parmgmc_amd import MGMC
    from parmgmc_amd.unstructured import build_hierarchy

    A = O.ex6_matrix(32, 1e-2)
    ops, ps = build_hierarchy(A.scipy().tocsr(), coarse_max=100)
    assert len(ops) >= 2
    mg = MGMC.from_hierarchy(ops, ps)
    mg.set_smoother(True, 1.0, 1, 1)  # -gamgmc_mg_levels_pc_mcgibbs_forward
    mg.setup()
    return A, mg


def mc_error(Sigma, nchains):
    """E ||C_N - Sigma||_F / ||Sigma||_F of N Gaussian samples"""
    f = np.linalg.norm(Sigma)
    return np.sqrt((f**2 + np.trace(Sigma) ** 2) / (nchains - 1)) / f


def test_ex6_shape_every_sample_index():
    """the configuration of tests/test_gpu_chains.py::test_ex6_shape_covariance, driven by sample_chains(cov=) with no Python
    in the loop: one error per sample index, the last one under that test's condition and equal to the host function on the
    final Y; stats= and cov= together leave the same bits in both"""
    import torch

    from parmgmc_amd import ChainCov, ChainStats, estimate_covariance_errors

    A, mg = _ex6_hierarchy()
    n, nchains, its = A.n, 1000, 40
    seeds = [0x5EED0000 + 7919 * c for c in range(nchains)]
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    cc = ChainCov.from_csr(A.rowptr, A.colidx, A.vals, nchains, max_steps=its)
    Y = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    mg.sample_chains(b, Y, its, seeds, cov=cc)
    errs = cc.errors()
    assert errs.shape == (its,) and cc.count() == its
    Ad = A.dense()
    Sigma = np.linalg.inv(Ad)
    mc_err = mc_error(Sigma, nchains)
    print("ex6 trace:", " ".join(f"{e:.4f}" for e in errs), f"mc_err {mc_err:.4f}")
    assert errs[-1] < min(2.0 * mc_err, 0.9), (errs, mc_err)
    Yh = Y.cpu().numpy()
    host = estimate_covariance_errors(A.rowptr, A.colidx, A.vals, Yh.T.copy(), nchains)
    bound = agreement_bound(Yh, host[0], cc.reference(), Ad)
    print(f"ex6 last index: device {errs[-1]:.15e} host {host[0]:.15e} diff {abs(errs[-1] - host[0]):.3e} / bound {bound:.3e}")
    assert abs(errs[-1] - host[0]) <= bound, (errs[-1], host[0], bound)
    # the samples are those of a run without any consumer
    Y0 = torch.zeros_like(Y)
    mg.sample_chains(b, Y0, its, seeds)
    assert torch.equal(Y0, Y)
    # stats= and cov= together
    qois = [None]
    cs1 = ChainStats(n, nchains, qois, max_steps=its)
    Y1 = torch.zeros_like(Y)
    mg.sample_chains(b, Y1, its, seeds, stats=cs1)
    cs2 = ChainStats(n, nchains, qois, max_steps=its)
    cc.reset()
    Y2 = torch.zeros_like(Y)
    mg.sample_chains(b, Y2, its, seeds, stats=cs2, cov=cc)
    assert torch.equal(Y1, Y) and torch.equal(Y2, Y)
    assert np.array_equal(cc.errors(), errs)
    (m1, v1), (m2, v2) = cs1.fields(), cs2.fields()
    assert torch.equal(m1, m2) and torch.equal(v1, v2)
    assert np.array_equal(cs1.trace(0), cs2.trace(0))
    with pytest.raises(ValueError):
        mg.sample_chains(b, Y2, 1, seeds, callback=lambda it, Yc: None, cov=cc)
    with pytest.raises(AssertionError):
        mg.sample_chains(b, Y2, 1, seeds, cov=ChainCov.from_dense(np.eye(n), nchains + 1, max_steps=1))


def test_ex6_shape_posterior_through_woodbury():
    """WoodburySampler.run_chains(cov=) on the three-observation set-up of tests/test_gpu_lowrank_chains.py: the error against
    (A + B S B^T)^-1 at every sample index, its last value under that test's condition (< 2 mc_err)"""
    import torch

    from parmgmc_amd import ChainCov
    from parmgmc_amd.wrappers import WoodburySampler

    A, mg = _ex6_hierarchy()
    n, nchains, its, cycles = A.n, 1000, 10, 20
    Ad = A.dense()
    B, S = _three_observations(n)
    post = np.linalg.inv(Ad + B @ np.diag(S) @ B.T)
    mc_err = mc_error(post, nchains)
    seeds = [0x5EED0000 + 7919 * c for c in range(nchains)]
    Ainv = dev(np.linalg.inv(Ad))

    def solve(rhs, x):
        x.copy_(Ainv @ rhs)

    wb = WoodburySampler(B, S, solve, lambda w, y, ctr: None, sample_chains=lambda W, Yc, ctr: mg.sample_chains(W, Yc, cycles, seeds, counter0=ctr * cycles))
    cc = ChainCov.from_csr(A.rowptr, A.colidx, A.vals, nchains, max_steps=its, lowrank=(B, S))
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    Y = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    wb.run_chains(b, Y, its, seeds, cov=cc)
    errs = cc.errors()
    assert errs.shape == (its,)
    print("woodbury trace:", " ".join(f"{e:.4f}" for e in errs), f"mc_err {mc_err:.4f}")
    assert errs[-1] < 2.0 * mc_err, (errs, mc_err)
    # the same number from the samples on the host
    Yh = Y.cpu().numpy()
    e_host = np.linalg.norm(np.cov(Yh) - post) / np.linalg.norm(post)
    bound = agreement_bound(Yh, e_host, cc.reference(), Ad + B @ np.diag(S) @ B.T)
    print(f"woodbury last index: device {errs[-1]:.15e} numpy {e_host:.15e} diff {abs(errs[-1] - e_host):.3e} / bound {bound:.3e}")
    assert abs(errs[-1] - e_host) <= bound, (errs[-1], e_host, bound)
    with pytest.raises(ValueError):
        wb.run_chains(b, Y, 1, seeds, callback=lambda it, Yc: None, cov=cc)
