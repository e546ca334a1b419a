"""Chain statistics on the device (pmg_chainstats_*): fields and traces against extended-precision numpy with bounds computed
from the inputs, bit-for-bit determinism, the ready-made C callbacks on the samplers, the bookkeeping calls, and an
ex7-shaped R-hat run."""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
ARG_OUTOFRANGE, ARG_WRONGSTATE = 63, 73
CONFIG4_ROWS = 377089  # rows of BASELINE config 4 (lshape.msh refined 5 times)


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def make_steps(n, C, T, offset, seed):
    """T steps of (n, C): unit-scale noise times a per-row scale in [0.1, 3], plus an offset"""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.1, 3.0, size=(n, 1))
    return [rng.standard_normal((n, C)) * scale + offset for _ in range(T)]


def make_qois(n, nqoi, seed):
    """the NULL (all ones) QOI first, then weight vectors"""
    rng = np.random.default_rng(seed + 99)
    return [None if q == 0 else rng.standard_normal(n) for q in range(nqoi)]


def check_against_longdouble(cs, steps, qois, label):
    """bounds of the issue, from the inputs alone"""
    T, (n, C) = len(steps), steps[0].shape
    mean, var = (t.cpu().numpy() for t in cs.fields())
    allY = np.concatenate(steps, axis=1).astype(np.longdouble)  # n x (T C)
    m_ref = allY.sum(axis=1) / (T * C)
    v_ref = ((allY - m_ref[:, None]) ** 2).sum(axis=1) / (T * C - 1)
    maxabs = float(np.abs(allY).max())
    mean_err = float(np.abs(mean - m_ref).max())
    mean_bound = T * C * EPS * maxabs
    var_err = float(np.abs(var - v_ref).max())
    var_bound = 16 * T * C * EPS * float((v_ref + m_ref**2).max())
    print(f"{label}: mean err {mean_err:.3e} / bound {mean_bound:.3e}; var err {var_err:.3e} / bound {var_bound:.3e}")
    assert mean_err <= mean_bound, (label, mean_err, mean_bound)
    assert var_err <= var_bound, (label, var_err, var_bound)
    g = n * EPS / (1 - n * EPS)
    for q, w in enumerate(qois):
        tr = cs.trace(q)
        assert tr.shape == (T, C)
        wl = np.ones(n, np.longdouble) if w is None else w.astype(np.longdouble)
        for t in range(T):
            Yl = steps[t].astype(np.longdouble)
            ref = wl @ Yl
            bound = g * (np.abs(wl)[:, None] * np.abs(Yl)).sum(axis=0)
            err = np.abs(tr[t] - ref)
            worst = float((err / bound).max())
            assert (err <= bound).all(), (label, q, t, worst)
        print(f"{label}: qoi {q} worst err / bound {worst:.3e}")


def run_steps(cs, steps):
    for Y in steps:
        cs.update(dev(Y))


SMALL = [(n, C, T, offset, nqoi) for n in (81, 1024) for C in (1, 3, 32, 65, 1000) for T, offset, nqoi in ((5, 0.0, 4), (3, 50.0, 1))] + [(81, 3, 4, 50.0, 0), (1024, 65, 2, 0.0, 0)]


@pytest.mark.parametrize("n,C,T,offset,nqoi", SMALL)
def test_fields_and_traces_small(n, C, T, offset, nqoi):
    from parmgmc_amd import ChainStats

    steps = make_steps(n, C, T, offset, seed=n + 7 * C + T)
    qois = make_qois(n, nqoi, seed=C)
    cs = ChainStats(n, C, qois, max_steps=T)
    run_steps(cs, steps)
    assert cs.count() == (T, T * C)
    check_against_longdouble(cs, steps, qois, f"n={n} C={C} T={T} offset={offset}")


@pytest.mark.parametrize("C,offset,nqoi", [(1, 50.0, 4), (32, 0.0, 1), (32, 50.0, 4), (1, 0.0, 0)])
def test_fields_and_traces_config4_size(C, offset, nqoi):
    from parmgmc_amd import ChainStats

    n, T = CONFIG4_ROWS, 4
    steps = make_steps(n, C, T, offset, seed=C + nqoi)
    qois = make_qois(n, nqoi, seed=C)
    cs = ChainStats(n, C, qois, max_steps=T)
    run_steps(cs, steps)
    check_against_longdouble(cs, steps, qois, f"config4 C={C} offset={offset}")


@pytest.mark.parametrize("n,C", [(1024, 3), (1024, 65), (CONFIG4_ROWS, 32), (5000, 200)])
def test_same_bits_twice(n, C):
    """the same updates after a reset, the second time on a non-default stream: the same bits"""
    import torch

    from parmgmc_amd import ChainStats

    steps = [dev(Y) for Y in make_steps(n, C, 3, 50.0, seed=C)]
    qois = make_qois(n, 2, seed=1)
    cs = ChainStats(n, C, qois, max_steps=3)
    for Y in steps:
        cs.update(Y)
    m1, v1 = cs.fields()
    t1 = [cs.trace(q) for q in range(2)]
    torch.cuda.synchronize()
    cs.reset()
    assert cs.count() == (0, 0)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for Y in steps:
            cs.update(Y)
        m2, v2 = cs.fields()
    st.synchronize()
    assert torch.equal(m1, m2) and torch.equal(v1, v2)
    for q in range(2):
        assert np.array_equal(t1[q], cs.trace(q))


def _compare_with_collected(cs, samples, qois, label):
    """the handle's statistics equal those of the collected samples within the bounds of check_against_longdouble"""
    steps = [s.reshape(s.shape[0], -1) for s in samples]
    check_against_longdouble(cs, steps, qois, label)


def _small_hierarchy():
    from parmgmc_amd import MGMC
    from parmgmc_amd.unstructured import build_hierarchy

    A = O.ex6_matrix(32, 1e-2)
    ops, ps = build_hierarchy(A.scipy().tocsr(), coarse_max=100)
    mg = MGMC.from_hierarchy(ops, ps)
    mg.set_smoother(True, 1.0, 1, 1)
    mg.setup()
    return A, mg


def test_sample_callback_single_chain():
    """C = 1 through pmg_chainstats_sample_callback on MGMC.sample: the statistics of the samples a Python callback collected
    from an identical run, and the samples themselves unchanged"""
    import torch

    from parmgmc_amd import ChainStats

    A, mg = _small_hierarchy()
    n, its = A.n, 12
    rng = np.random.default_rng(3)
    b = dev(rng.standard_normal(n))
    qois = [None, rng.standard_normal(n)]
    got = []
    y1 = torch.zeros(n, dtype=torch.float64, device="cuda")
    mg.sample(b, y1, its, seed=0xBEEF, callback=lambda it, y: got.append(y.cpu().numpy().copy()))
    cs = ChainStats(n, 1, qois, max_steps=its)
    y2 = torch.zeros(n, dtype=torch.float64, device="cuda")
    mg.sample(b, y2, its, seed=0xBEEF, stats=cs)
    assert torch.equal(y1, y2)
    assert cs.count() == (its, its)
    _compare_with_collected(cs, got, qois, "MGMC.sample stats=")
    with pytest.raises(ValueError):
        mg.sample(b, y2, 1, seed=1, callback=lambda it, y: None, stats=cs)


def test_chains_callback_on_mgmc_chains():
    import torch

    from parmgmc_amd import ChainStats

    A, mg = _small_hierarchy()
    n, its, nchains = A.n, 6, 8
    seeds = [0xCAFE + 977 * c for c in range(nchains)]
    rng = np.random.default_rng(4)
    b = dev(rng.standard_normal(n))
    qois = [None, rng.standard_normal(n)]
    got = []
    Y0 = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    mg.sample_chains(b, Y0, its, seeds)  # no callback at all
    Y1 = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    mg.sample_chains(b, Y1, its, seeds, callback=lambda it, Y: got.append(Y.cpu().numpy().copy()))
    cs = ChainStats(n, nchains, qois, max_steps=its)
    Y2 = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    mg.sample_chains(b, Y2, its, seeds, stats=cs)
    assert torch.equal(Y0, Y2) and torch.equal(Y1, Y2)
    assert cs.count() == (its, its * nchains)
    _compare_with_collected(cs, got, qois, "MGMC.sample_chains stats=")
    with pytest.raises(ValueError):
        mg.sample_chains(b, Y2, 1, seeds, callback=lambda it, Y: None, stats=cs)
    # a handle of other sizes is refused by the wrapper before the library is called
    with pytest.raises(AssertionError):
        mg.sample_chains(b, Y2, 1, seeds, stats=ChainStats(n, nchains + 1, [], max_steps=1))


def test_stats_on_woodbury_run_chains():
    import torch

    from parmgmc_amd import ChainStats
    from parmgmc_amd.wrappers import WoodburySampler

    A, mg = _small_hierarchy()
    n, its, nchains = A.n, 5, 8
    seeds = [0xCAFE + 977 * c for c in range(nchains)]
    rng = np.random.default_rng(5)
    B = np.zeros((n, 2))
    B[rng.choice(n, 40, replace=False), 0] = 1.0 / 40
    B[rng.choice(n, 30, replace=False), 1] = 1.0 / 30
    S = np.array([50.0, 80.0])
    Ainv = dev(np.linalg.inv(A.scipy().toarray()))

    def solve(rhs, x):
        x.copy_(Ainv @ rhs)

    wb = WoodburySampler(B, S, solve, lambda w, y, ctr: None, sample_chains=lambda W, Yc, ctr: mg.sample_chains(W, Yc, 1, seeds, counter0=ctr))
    b = dev(rng.standard_normal(n))
    qois = [rng.standard_normal(n), None]
    got = []
    Y1 = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    wb.run_chains(b, Y1, its, seeds, callback=lambda it, Y: got.append(Y.cpu().numpy().copy()))
    cs = ChainStats(n, nchains, qois, max_steps=its)
    Y2 = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    wb.run_chains(b, Y2, its, seeds, stats=cs)
    assert torch.equal(Y1, Y2)
    _compare_with_collected(cs, got, qois, "WoodburySampler.run_chains stats=")
    with pytest.raises(ValueError):
        wb.run_chains(b, Y2, 1, seeds, callback=lambda it, Y: None, stats=cs)


def test_reset_overflow_and_windows():
    import torch

    from parmgmc_amd import ChainStats, PMGError, gelman_rubin

    n, C_, T = 300, 5, 4
    steps = make_steps(n, C_, T, 0.0, seed=11)
    cs = ChainStats(n, C_, [None], max_steps=T)
    with pytest.raises(PMGError) as e:
        cs.fields()
    assert e.value.code == ARG_WRONGSTATE
    run_steps(cs, steps)
    with pytest.raises(PMGError) as e:  # max_steps updates have been made
        cs.update(dev(steps[0]))
    assert e.value.code == ARG_OUTOFRANGE
    assert cs.count() == (T, T * C_)
    full = cs.trace(0)
    assert np.array_equal(cs.trace(0, 1, 2), full[1:3])
    assert cs.trace(0, T, 0).shape == (0, C_)
    for q, first, count in ((0, 0, T + 1), (0, T, 1), (0, -1, 1), (1, 0, 1), (0, 3, 2)):
        with pytest.raises(PMGError) as e:
            cs.trace(q, first, count)
        assert e.value.code == ARG_OUTOFRANGE
    for first, count in ((0, 1), (3, 2), (0, T + 1)):
        with pytest.raises(PMGError) as e:
            cs.rhat(0, first, count)
        assert e.value.code == ARG_OUTOFRANGE
    # the device R-hat is pmg_gelman_rubin on the trace copied out: exact
    assert cs.rhat(0, 1, 3) == gelman_rubin(full[1:4].T)
    assert cs.rhat(0) == gelman_rubin(full.T)
    # reset forgets everything: the statistics of the later steps alone
    cs.reset()
    assert cs.count() == (0, 0)
    with pytest.raises(PMGError) as e:
        cs.fields()
    assert e.value.code == ARG_WRONGSTATE
    with pytest.raises(PMGError):
        cs.trace(0, 0, 1)
    run_steps(cs, steps[2:])
    check_against_longdouble(cs, steps[2:], [None], "after reset")
    # one chain: two steps are two samples; iact runs per chain
    cs1 = ChainStats(n, 1, [None], max_steps=600)
    cs1.update(dev(steps[0][:, :1]))
    with pytest.raises(PMGError) as e:
        cs1.fields()
    assert e.value.code == ARG_WRONGSTATE
    rng = np.random.default_rng(0)
    for _ in range(599):
        cs1.update(dev(rng.standard_normal((n, 1))))
    (tau, valid), = cs1.iact(0)
    assert 0.5 < tau < 2.0, (tau, valid)  # independent draws: tau = 1
    torch.cuda.synchronize()


CHECK_EVERY, BURN_IN, WINDOW = 50, 50, 200


def test_ex7_shape_rhat():
    """examples/ex7.c on the ~1000-row ex6 operator: 8 chains started overdispersed (1e6 * noise, ex7.c:176), all-ones QOI
    (VecSum, ex7.c:46), fixed seeds.  The forward Gibbs sampler over its first check_every = 50 steps has not converged by
    ex7's criterion R_crit = 1.05; MGMC over 200 steps after a burn-in of 50 has.
    Observed on the MI355X: R-hat 180.54 (Gibbs), 1.00368 (MGMC)."""
    import torch

    from parmgmc_amd import MCSOR, ChainStats, gelman_rubin, vec_set_random_standard_normal

    A, mg = _small_hierarchy()
    n, nchains, R_crit = A.n, 8, 1.05
    seeds = [0xE7 + 7919 * c for c in range(nchains)]
    b = torch.zeros(n, dtype=torch.float64, device="cuda")

    def start():
        Y = torch.empty((nchains, n), dtype=torch.float64, device="cuda")
        for c in range(nchains):
            vec_set_random_standard_normal(Y[c], seed=0x57A27 + c)
        return (1e6 * Y).T.contiguous()

    # Gibbs: MCSOR.sample_chains has no callback, update between the calls
    mc = MCSOR(A.rowptr, A.colidx, A.vals).setup()
    cs = ChainStats(n, nchains, [None], max_steps=CHECK_EVERY)
    Y = start()
    for it in range(CHECK_EVERY):
        mc.sample_chains(b, Y, 1, seeds, counter0=it)
        cs.update(Y)
    r_gibbs = cs.rhat(0, 0, CHECK_EVERY)
    assert r_gibbs == gelman_rubin(cs.trace(0).T)
    # MGMC: burn-in, reset, then the window through the C callback
    csm = ChainStats(n, nchains, [None], max_steps=max(BURN_IN, WINDOW))
    Y = start()
    ctr = mg.sample_chains(b, Y, BURN_IN, seeds, stats=csm)
    csm.reset()
    mg.sample_chains(b, Y, WINDOW, seeds, counter0=ctr, stats=csm)
    r_mgmc = csm.rhat(0, 0, WINDOW)
    assert r_mgmc == gelman_rubin(csm.trace(0).T)
    print(f"ex7 shape: R-hat Gibbs first {CHECK_EVERY} = {r_gibbs:.6g}, MGMC {WINDOW} after {BURN_IN} = {r_mgmc:.6g}")
    assert r_gibbs > R_crit, r_gibbs
    assert r_mgmc < R_crit, r_mgmc
