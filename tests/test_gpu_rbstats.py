"""Rao-Blackwellised chain statistics on the device (pmg_rbstats_*): conditional means against extended-precision numpy with
forward-error bounds computed from the inputs (tests/rbstats_cases.py), exact results where nothing rounds, the order contract
against ChainStats fed the same conditional means, the fields against np.longdouble, the wiring into the samplers, the
stream contract, and the end-to-end comparison of the two estimators on an MGMC run."""
import ctypes as C

import numpy as np
import pytest

import rbstats_cases as R

pytestmark = pytest.mark.gpu
ARG_WRONGSTATE, ARG_SIZ = 73, 60


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def make_rb(M, C_, lr=None, b=None):
    from parmgmc_amd import RBStats

    return RBStats((M.rowptr, M.colidx, M.vals), C_, lowrank=lr, b=None if b is None else dev(b))


MATRICES = {M.name: M for M in R.matrices()}
INTEGER = {M.name: M for M in R.integer_matrices()}


# ---- 1: cond_mean over the case table -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", R.CHAINS + R.MORE_CHAINS)
@pytest.mark.parametrize("name", list(MATRICES))
def test_cond_mean_against_longdouble(name, C_):
    """every rank of the table on one handle, with and without a right-hand side.
    Observed on the MI355X: worst |m - ref| / bound over the whole table 0.29 (k = 0), 0.18 (k > 0)."""
    M = MATRICES[name]
    Y = R.samples(M.n, C_, seed=M.n + C_)
    b = R.rhs(M.n, seed=C_)
    rb = make_rb(M, C_)
    Yd = dev(Y)
    for k in R.RANKS:
        lr = R.lowrank(M.n, k, seed=M.n)
        rb.set_lowrank(*(lr or (None, None)))
        for rhs_ in (b, None):
            rb.set_rhs(None if rhs_ is None else dev(rhs_))
            got = host(rb.cond_mean(Yd))
            ref, bound = R.cond_mean_ref(M, Y, rhs_, lr)
            err = np.abs(got.astype(np.longdouble) - ref)
            worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))))
            print(f"{name} C={C_} k={k} b={'yes' if rhs_ is not None else 'zero'}: worst err / bound {worst:.3f}")
            assert np.isfinite(got).all()
            assert (err <= bound).all(), (name, C_, k, worst)
    assert rb.count() == (0, 0)  # cond_mean records nothing


@pytest.mark.parametrize("C_", R.CHAINS + R.MORE_CHAINS)
@pytest.mark.parametrize("name", list(INTEGER))
def test_cond_mean_exact_on_integer_data(name, C_):
    """k = 0, integer off-diagonal entries, y and b, power-of-two diagonal: no operation rounds, the result is the exact one"""
    M = INTEGER[name]
    Y = R.samples(M.n, C_, seed=C_, integer=True)
    b = R.rhs(M.n, seed=C_, integer=True)
    ref, bound = R.cond_mean_ref(M, Y, b)
    want = ref.astype(np.float64)
    assert np.array_equal(want.astype(np.longdouble), ref)  # the exact result is a float64
    got = host(make_rb(M, C_, b=b).cond_mean(dev(Y)))
    assert np.array_equal(got, want)
    assert (got[3] == b[3, None] / R.cond_precision_host(M)[3]).all()  # the isolated row


# ---- 2: a diagonal Q ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", R.CHAINS + R.MORE_CHAINS)
def test_diagonal_matrix(C_):
    """m = b / q for every sample: mean == b / q, M2 == 0 and var == 1 / q bit for bit after 1, 2 and 5 updates.  The mean of C
    equal values is formed as (tree sum) / C, which returns the value bit for bit when C x is exact: dyadic data (integer b,
    power-of-two q) for every C of the table, and any data where the sums only double (C a power of two, or chunks of 64, 1, 2)."""
    from parmgmc_amd import PMGError

    n = 67
    for dyadic in (True, False):
        if not dyadic and C_ not in (1, 2, 8, 64, 65, 130, 4, 16, 32, 128):
            continue
        M = R.diagonal(n, seed=C_, dyadic=dyadic)
        b = R.rhs(n, seed=C_, integer=dyadic)
        q = R.cond_precision_host(M)
        rb = make_rb(M, C_, b=b)
        done = 0
        for updates in (1, 2, 5):
            while done < updates:
                rb.update(dev(R.samples(n, C_, seed=100 * C_ + done)))
                done += 1
            if done * C_ < 2:
                with pytest.raises(PMGError) as e:
                    rb.fields()
                assert e.value.code == ARG_WRONGSTATE
                continue
            mean, var = (host(t) for t in rb.fields())
            assert np.array_equal(mean, b / q), (dyadic, updates)
            assert np.array_equal(var, 1.0 / q), (dyadic, updates)  # 1 / q + 0.0 / (N - 1)
        assert rb.count() == (5, 5 * C_)


# ---- 3: the order contract ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,C_,k", [("ex6", 3, 0), ("spd65", 8, 3), ("spd257", 65, 1), ("spd65", 130, 0), ("one", 5, 0), ("ex6", 1, 5)])
def test_order_contract_against_chainstats(name, C_, k):
    """the fields after S steps are those of a ChainStats fed the cond_mean outputs of the same steps: the same mean bit for bit,
    var = 1 / q + (ChainStats var) with the two roundings as written; the same bits after a reset on another stream and in a
    fresh handle"""
    import torch

    from parmgmc_amd import ChainStats

    M = MATRICES[name]
    S_ = 4
    lr = R.lowrank(M.n, k, seed=3)
    b = R.rhs(M.n, seed=k)
    steps = [dev(R.samples(M.n, C_, seed=10 * C_ + s)) for s in range(S_)]
    rb = make_rb(M, C_, lr, b)
    cs = ChainStats(M.n, C_, [], max_steps=S_)
    for Y in steps:
        cs.update(rb.cond_mean(Y))
        rb.update(Y)
    mean, var = rb.fields()
    cmean, cvar = cs.fields()
    q = R.cond_precision_host(M, lr)
    assert torch.equal(mean, cmean)
    assert np.array_equal(host(var), 1.0 / q + host(cvar))
    torch.cuda.synchronize()
    rb.reset()
    assert rb.count() == (0, 0)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for Y in steps:
            rb.update(Y)
        mean2, var2 = rb.fields()
    st.synchronize()
    assert torch.equal(mean, mean2) and torch.equal(var, var2)
    fresh = make_rb(M, C_, lr, b)
    for Y in steps:
        fresh.update(Y)
    mean3, var3 = fresh.fields()
    assert torch.equal(mean, mean3) and torch.equal(var, var3)


# ---- 4: the fields against np.longdouble --------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", R.CHAINS + R.MORE_CHAINS)
@pytest.mark.parametrize("name,k", [("ex6", 0), ("spd65", 3), ("spd257", 0), ("one", 1)])
def test_fields_against_longdouble(name, k, C_):
    """three updates; the reference and the bounds of rbstats_cases.fields_reference.
    Observed on the MI355X: worst mean err / bound 0.072, worst var err / bound 0.056."""
    M = MATRICES[name]
    T = 3
    lr = R.lowrank(M.n, k, seed=5)
    b = R.rhs(M.n, seed=3 * C_)
    steps = [R.samples(M.n, C_, seed=7 * C_ + s) for s in range(T)]
    rb = make_rb(M, C_, lr, b)
    for Y in steps:
        rb.update(dev(Y))
    assert rb.count() == (T, T * C_)
    mean, var = (host(t) for t in rb.fields())
    refs = [R.cond_mean_ref(M, Y, b, lr) for Y in steps]
    m_ref, v_ref, mean_bound, var_bound = R.fields_reference([r[0] for r in refs], [r[1] for r in refs], R.cond_precision_host(M, lr))
    mean_err, var_err = np.abs(mean - m_ref), np.abs(var - v_ref)
    print(f"{name} k={k} C={C_}: mean err / bound {float((mean_err / mean_bound).max()):.3e}; var err / bound {float((var_err / var_bound).max()):.3e}")
    assert (mean_err <= mean_bound).all()
    assert (var_err <= var_bound).all()


# ---- 5: the wiring into the samplers --------------------------------------------------------------------------------------------
def _small_hierarchy():
    from parmgmc_amd import MGMC

    A, ops, ps, b = R.e2e_problem()
    mg = MGMC.from_hierarchy(ops, ps)
    mg.set_smoother(True, 1.0, 1, 1)
    mg.setup()
    return A, mg, b


def _by_hand(A, nchains, b, collected, lr=None):
    """an RBStats updated by hand on the samples a Python callback received"""
    rb = make_rb(R.Matrix("A", A.rowptr, A.colidx, A.vals, A.n, ""), nchains, lr, b)
    for Y in collected:
        rb.update(Y)
    return rb


def _same_fields(x, y):
    import torch

    assert x.count() == y.count()
    for s, t in zip(x.fields(), y.fields()):
        assert bool(torch.isfinite(s).all()) and torch.equal(s, t)


def test_wiring_mgmc_sample_chains_with_stats_and_rb():
    import torch

    from parmgmc_amd import ChainStats, RBStats

    A, mg, b = _small_hierarchy()
    n, its, nchains = A.n, 6, 8
    seeds = R.E2E["seeds"]
    bd = dev(b)
    got = []
    Y1 = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    mg.sample_chains(bd, Y1, its, seeds, callback=lambda it, Y: got.append(Y.clone()))
    want_rb = _by_hand(A, nchains, b, got)
    want_cs = ChainStats(n, nchains, [], max_steps=its)
    for Y in got:
        want_cs.update(Y)
    # both together, then rb= alone through the library's own callback
    rb, cs = RBStats(A, nchains, b=bd), ChainStats(n, nchains, [], max_steps=its)
    Y2 = torch.zeros_like(Y1)
    mg.sample_chains(bd, Y2, its, seeds, rb=rb, stats=cs)
    assert torch.equal(Y1, Y2)
    _same_fields(rb, want_rb)
    _same_fields(cs, want_cs)
    rb2 = RBStats(A, nchains, b=bd)
    Y3 = torch.zeros_like(Y1)
    mg.sample_chains(bd, Y3, its, seeds, rb=rb2)
    assert torch.equal(Y1, Y3)
    _same_fields(rb2, want_rb)
    with pytest.raises(ValueError):
        mg.sample_chains(bd, Y3, 1, seeds, callback=lambda it, Y: None, rb=rb2)
    with pytest.raises(AssertionError):  # the wrapper refuses other sizes before the library is called
        mg.sample_chains(bd, Y3, 1, seeds, rb=RBStats(A, nchains + 1))
    # the library's callback refuses them too
    from parmgmc_amd.capi import lib

    other = RBStats(A, nchains + 1)
    assert lib.pmg_rbstats_callback(0, C.c_void_p(Y3.data_ptr()), n, nchains, other._h) == ARG_SIZ
    assert lib.pmg_rbstats_callback(0, C.c_void_p(Y3.data_ptr()), n + 1, nchains + 1, other._h) == ARG_SIZ
    assert other.count() == (0, 0)


def test_wiring_mgmc_sample_single_chain():
    import torch

    from parmgmc_amd import ChainStats, RBStats

    A, mg, b = _small_hierarchy()
    n, its = A.n, 7
    bd = dev(b)
    got = []
    y1 = torch.zeros(n, dtype=torch.float64, device="cuda")
    mg.sample(bd, y1, its, seed=0xBEEF, callback=lambda it, y: got.append(y.clone()))
    want = _by_hand(A, 1, b, got)
    rb = RBStats(A, 1, b=bd)
    y2 = torch.zeros_like(y1)
    mg.sample(bd, y2, its, seed=0xBEEF, rb=rb)
    assert torch.equal(y1, y2)
    _same_fields(rb, want)
    rb3, cs = RBStats(A, 1, b=bd), ChainStats(n, 1, [], max_steps=its)
    y3 = torch.zeros_like(y1)
    mg.sample(bd, y3, its, seed=0xBEEF, rb=rb3, stats=cs)
    assert torch.equal(y1, y3) and cs.count() == (its, its)
    _same_fields(rb3, want)
    with pytest.raises(ValueError):
        mg.sample(bd, y3, 1, seed=1, callback=lambda it, y: None, rb=rb3)


def test_wiring_woodbury_run_chains():
    """the handle is built on (A, B, S): the conditional means are those of the posterior precision A + B S B^T"""
    import torch

    from parmgmc_amd import RBStats
    from parmgmc_amd.wrappers import WoodburySampler

    A, mg, b = _small_hierarchy()
    n, its, nchains = A.n, 5, 8
    seeds = R.E2E["seeds"]
    rng = np.random.default_rng(5)
    B = np.zeros((n, 2))
    B[rng.choice(n, 40, replace=False), 0] = 1.0 / 40
    B[rng.choice(n, 30, replace=False), 1] = 1.0 / 30
    S = np.array([50.0, 80.0])
    Ainv = dev(np.linalg.inv(A.scipy().toarray()))

    def solve(rhs_, x):
        x.copy_(Ainv @ rhs_)

    wb = WoodburySampler(B, S, solve, lambda w, y, ctr: None, sample_chains=lambda W, Yc, ctr: mg.sample_chains(W, Yc, 1, seeds, counter0=ctr))
    bd = dev(b)
    got = []
    Y1 = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    wb.run_chains(bd, Y1, its, seeds, callback=lambda it, Y: got.append(Y.clone()))
    want = _by_hand(A, nchains, b, got, lr=(B, S))
    rb = RBStats(A, nchains, lowrank=(B, S), b=bd)
    Y2 = torch.zeros_like(Y1)
    wb.run_chains(bd, Y2, its, seeds, rb=rb)
    assert torch.equal(Y1, Y2)
    _same_fields(rb, want)
    # and they are the conditional means of the posterior: m == y + (b - Q y) / q
    Q = R.dense(R.Matrix("A", A.rowptr, A.colidx, A.vals, A.n, ""), (np.asfortranarray(B), S))
    Yl = host(Y2).astype(np.longdouble)
    ident = Yl + (b.astype(np.longdouble)[:, None] - Q @ Yl) / np.diag(Q)[:, None]
    assert float(np.abs(host(rb.cond_mean(Y2)) - ident).max()) < 1e-10 * float(np.abs(ident).max())
    with pytest.raises(ValueError):
        wb.run_chains(bd, Y2, 1, seeds, callback=lambda it, Y: None, rb=rb)


# ---- 6: end to end ------------------------------------------------------------------------------------------------------------
def test_end_to_end_rb_beats_plain_moments():
    """8 chains of MGMC on the ~1000-row ex6 operator, stats= and rb= together after the burn-in: the Rao-Blackwellised fields
    are no further from the exact mean and diag(Sigma) (pmg_chaincov_get_reference of a pmg_chol handle) than the plain moments.
    The configuration (rbstats_cases.E2E) was fixed from the oracle's chain on the CPU, where err_rb / err_plain <= 0.9 for
    both fields (tests/test_rbstats_cases.py asserts it; the figures are in its docstring and in DESIGN 11.5).
    Observed on the MI355X: variance err_plain 0.07981, err_rb 0.06119; mean err_plain 0.03060, err_rb 0.02646 (the figures of
    the oracle's chain on the CPU to all digits shown)."""
    import torch

    from parmgmc_amd import ChainStats, RBStats
    from parmgmc_amd.wrappers import ChainCov

    E = R.E2E
    A, mg, b = _small_hierarchy()
    n, nchains = A.n, E["nchains"]
    bd = dev(b)
    Sigma = ChainCov.from_csr(A.rowptr, A.colidx, A.vals, nchains, max_steps=1).reference()
    mu = Sigma @ b
    cs, rb = ChainStats(n, nchains, [], max_steps=max(E["burn_in"], E["window"])), RBStats(A, nchains, b=bd)
    Y = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    ctr = mg.sample_chains(bd, Y, E["burn_in"], E["seeds"], stats=cs, rb=rb)
    cs.reset()
    rb.reset()
    mg.sample_chains(bd, Y, E["window"], E["seeds"], counter0=ctr, stats=cs, rb=rb)
    assert cs.count() == rb.count() == (E["window"], E["window"] * nchains)
    (pm, pv), (rm, rv) = ((host(t) for t in x.fields()) for x in (cs, rb))
    vp, vr = R.rel2(pv, np.diag(Sigma)), R.rel2(rv, np.diag(Sigma))
    mp, mr = R.rel2(pm, mu), R.rel2(rm, mu)
    print(f"end to end: variance err_plain {vp:.5f} err_rb {vr:.5f}; mean err_plain {mp:.5f} err_rb {mr:.5f}")
    assert vr <= vp, (vr, vp)
    assert mr <= mp, (mr, mp)


# ---- 7: the stream contract -----------------------------------------------------------------------------------------------------
def test_stream_contract():
    """a fresh handle whose first device call is on a side stream gives the bits of a twin on the default stream, and update,
    cond_mean and get_fields return while the stream is still busy with what was queued before them (no host synchronisation)"""
    import torch

    M = MATRICES["spd257"]
    C_, T = 8, 3
    lr = R.lowrank(M.n, 3, seed=1)
    b = R.rhs(M.n, seed=1)
    steps = [dev(R.samples(M.n, C_, seed=s)) for s in range(T)]
    a = torch.randn((4096, 4096), dtype=torch.float64, device="cuda") / 64.0
    scratch = torch.empty_like(a)
    torch.mm(a, a, out=scratch)
    torch.cuda.synchronize()

    def run(rb):
        for Y in steps:
            rb.update(Y)
        return rb.fields() + (rb.cond_mean(steps[0]),)

    side_h, twin_h, warm = make_rb(M, C_, lr, b), make_rb(M, C_, lr, b), make_rb(M, C_, lr, b)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        side = run(side_h)
    st.synchronize()
    twin = run(twin_h)
    torch.cuda.synchronize()
    for s, t in zip(side, twin):
        assert bool(torch.isfinite(s).all()) and torch.equal(s, t)
    # steady state: the handle is warm (its device memory is there), the producer is slow, the poisoned input is filled behind it
    run(warm)
    warm.reset()
    torch.cuda.synchronize()
    Yp = [torch.full_like(Y, float("nan")) for Y in steps]
    busy = torch.cuda.Event()
    with torch.cuda.stream(st):
        for _ in range(24):
            torch.mm(a, a, out=scratch)
        busy.record()
        for p, Y in zip(Yp, steps):
            p.copy_(Y, non_blocking=True)
        got = None
        for p in Yp:
            warm.update(p)
        got = warm.fields() + (warm.cond_mean(Yp[0]),)
        returned_early = not busy.query()
    st.synchronize()
    assert returned_early, "the calls returned after the producer had finished: they synchronise the host, or the delay is too short"
    for s, t in zip(got, twin):
        assert torch.equal(s, t)
