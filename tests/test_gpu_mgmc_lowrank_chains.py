"""Many chains per call of MGMC on a hierarchy with a low-rank (MATLRC) update (pmg_mgmc_set_lowrank + pmg_mgmc_sample_chains /
pmg_mgmc_sample_chains_rhs): column c of every chains call equals, bit for bit (torch.equal), pmg_mgmc_sample on that column
alone with seed = seeds[c] (and b = B[:, c] for the per-chain right-hand sides), in both storage forms of the update, with
either coarse sampler, correction form and guesszero setting; resume, seeds, interleaving with single-chain calls, callbacks,
side streams and the byte model; last, the ex6-shaped posterior covariance over 1000 chains with ONE cycle per step."""
import numpy as np
import pytest

import lrc_chain_workloads as W
from lrc_chain_workloads import config4, delay, streams  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
SWEEP_CONFIGS = {"om1_scaled_fwd": (1.0, True, 1), "om1_unscaled_fwd": (1.0, False, 1), "om1.3_scaled_sym": (1.3, True, 3)}  # (omega, scaled, sweep type)


def _compare(mg, n, nchains, rng, its=2, counter0=3, forms=((False, False), (False, True), (True, False), (True, True)), per_chain=(False, True)):
    """chains call against the single-chain call on every column, for the shared b and one b per chain"""
    import torch

    seeds = W.SEEDS[:nchains]
    for literal, guesszero in forms:
        mg.set_correction_form(literal)
        for rhs in per_chain:
            b = W.dev(rng.standard_normal((n, nchains) if rhs else n))
            b_keep = b.clone()
            Y0 = W.dev(rng.standard_normal((n, nchains)))
            Y = Y0.clone()
            ctr = mg.sample_chains(b, Y, its, seeds, counter0=counter0, guesszero=guesszero)
            assert ctr == counter0 + its
            assert torch.equal(b, b_keep), "the right-hand side changed"
            for c in range(nchains):
                y = Y0[:, c].contiguous()
                bc = b[:, c].contiguous() if rhs else b
                assert mg.sample(bc, y, its, seeds[c], counter0=counter0, guesszero=guesszero) == ctr
                assert torch.equal(Y[:, c], y), (literal, guesszero, rhs, c)
            assert torch.equal(b, b_keep)
    mg.set_correction_form(False)


@pytest.mark.parametrize("cfg", list(SWEEP_CONFIGS))
@pytest.mark.parametrize("coarse", ["cholsampler", "gibbs"])
@pytest.mark.parametrize("nchains,k", [(1, 1), (3, 17), (32, 3), (65, 64)])
@pytest.mark.parametrize("form", ["rows", "wide"])
def test_mgmc_lowrank_chains_small(form, nchains, k, coarse, cfg):
    A, ops, ps = W.hierarchy_17()
    omega, scaled, sweep = SWEEP_CONFIGS[cfg]
    mg = W.make_mgmc(ops, ps, W.observations_17(form, k, 10 * k + nchains), coarse, omega, scaled, sweep)
    top = len(ops) - 1
    kk, rows, dense = W.level_lowrank_sizes(mg, ops, top)
    assert kk == k and dense == (form == "wide")
    if form == "rows":  # one block of support rows: the one-workgroup form runs on the fine level
        assert 0 < rows <= W.ROWS_PER_BLOCK
    _compare(mg, A.n, nchains, np.random.default_rng(k * nchains))


def _config4_mgmc(config4, coloring, sweep):  # noqa: F811
    A, ops, ps, B, S, cache = config4
    if (coloring, sweep) not in cache:
        cache[(coloring, sweep)] = W.make_mgmc(ops, ps, (B, S), "cholsampler", sweep=sweep, coloring=coloring)
    return cache[(coloring, sweep)]


@pytest.mark.parametrize("nchains", [1, 8, 32])
@pytest.mark.parametrize("sweep", [1, 3], ids=["forward", "symmetric"])
@pytest.mark.parametrize("coloring", ["greedy", "iterated"])
def test_mgmc_lowrank_chains_config4(config4, coloring, sweep, nchains):  # noqa: F811
    """several 1024-row blocks of support rows on the fine level and the one below (three launches per repair), one block
    (the one-workgroup form) further down"""
    from parmgmc_amd import COLORING_GREEDY, COLORING_ITERATED

    A, ops, _, _, _, _ = config4
    mg = _config4_mgmc(config4, COLORING_ITERATED if coloring == "iterated" else COLORING_GREEDY, sweep)
    top = len(ops) - 1
    support = [W.level_lowrank_sizes(mg, ops, l) for l in range(1, top + 1)]  # (k, rows, dense) of the levels above the exact coarse sampler
    assert not support[-1][2] and support[-1][1] > 2 * W.ROWS_PER_BLOCK
    assert any(not dense and 0 < ns <= W.ROWS_PER_BLOCK for _, ns, dense in support[:-1]), support
    _compare(mg, A.shape[0], nchains, np.random.default_rng(nchains), forms=((False, False),), per_chain=(False,))


def _small(form="rows", k=3, coarse="gibbs", sweep=3, lowrank=True):
    A, ops, ps = W.hierarchy_17()
    return A, W.make_mgmc(ops, ps, W.observations_17(form, k, 77) if lowrank else None, coarse, 1.0, True, sweep)


@pytest.mark.parametrize("form", ["rows", "wide"])
def test_resume_and_equal_seeds(form):
    import torch

    A, mg = _small(form)
    rng = np.random.default_rng(1)
    seeds = list(W.SEEDS[:8])
    seeds[5] = seeds[2]
    b = W.dev(rng.standard_normal(A.n))
    Y0 = W.dev(rng.standard_normal((A.n, 8)))
    Y0[:, 5] = Y0[:, 2]
    Ya, Yb = Y0.clone(), Y0.clone()
    c1 = mg.sample_chains(b, Ya, 2, seeds, counter0=11)
    assert c1 == 13 and mg.sample_chains(b, Ya, 2, seeds, counter0=c1) == 15
    assert mg.sample_chains(b, Yb, 4, seeds, counter0=11) == 15
    assert torch.equal(Ya, Yb)
    assert torch.equal(Ya[:, 5], Ya[:, 2]) and not torch.equal(Ya[:, 4], Ya[:, 2])


@pytest.mark.parametrize("form", ["rows", "wide"])
@pytest.mark.parametrize("coarse", ["cholsampler", "gibbs"])
def test_interleaved_with_single_chain_calls(form, coarse):
    """single, chains, single, chains on one handle: each call gives the bits it gives on a handle of its own"""
    import torch

    rng = np.random.default_rng(2)
    A, mg = _small(form, coarse=coarse)
    n, nchains = A.n, 5
    b = W.dev(rng.standard_normal(n))
    y0, Y0 = W.dev(rng.standard_normal(n)), W.dev(rng.standard_normal((n, nchains)))
    seeds = W.SEEDS[:nchains]

    def single(h, y_in, ctr):
        y = y_in.clone()
        h.sample(b, y, 2, 0xABCD, counter0=ctr)
        return y

    def chains(h, Y_in, ctr):
        Y = Y_in.clone()
        h.sample_chains(b, Y, 2, seeds, counter0=ctr)
        return Y

    s1 = single(mg, y0, 0)
    c1 = chains(mg, Y0, 0)
    s2 = single(mg, s1, 2)
    c2 = chains(mg, c1, 2)
    assert torch.equal(s1, single(_small(form, coarse=coarse)[1], y0, 0))
    assert torch.equal(c1, chains(_small(form, coarse=coarse)[1], Y0, 0))
    assert torch.equal(s2, single(_small(form, coarse=coarse)[1], s1, 2))
    assert torch.equal(c2, chains(_small(form, coarse=coarse)[1], c1, 2))
    assert not torch.equal(s2, s1) and not torch.equal(c2, c1)


def test_callback_stats_and_cov():
    import torch

    from parmgmc_amd import ChainStats
    from parmgmc_amd.wrappers import ChainCov

    A, ops, ps = W.hierarchy_17()
    lowrank = W.observations_17("rows", 3, 5)
    mg = W.make_mgmc(ops, ps, lowrank, "cholsampler")
    n, nchains, its = A.n, 8, 3
    rng = np.random.default_rng(3)
    b, Y0 = W.dev(rng.standard_normal(n)), W.dev(rng.standard_normal((n, nchains)))
    w = rng.standard_normal(n)
    seeds = W.SEEDS[:nchains]
    # a Python loop over the steps
    steps, Y = [], Y0.clone()
    cs_loop = ChainStats(n, nchains, [None, w], max_steps=its)
    cov_loop = ChainCov.from_csr(A.rowptr, A.colidx, A.vals, nchains, max_steps=its, lowrank=lowrank)
    for it in range(its):
        assert mg.sample_chains(b, Y, 1, seeds, counter0=it) == it + 1
        steps.append(Y.clone())
        cs_loop.update(Y)
        cov_loop.update(Y)
    # the callback sees every step
    seen, Yc = [], Y0.clone()
    mg.sample_chains(b, Yc, its, seeds, callback=lambda it, Yit: seen.append((it, Yit.clone())))
    assert [it for it, _ in seen] == list(range(its))
    for (_, got), want in zip(seen, steps):
        assert torch.equal(got, want)
    # stats= and cov=
    cs, Ys = ChainStats(n, nchains, [None, w], max_steps=its), Y0.clone()
    mg.sample_chains(b, Ys, its, seeds, stats=cs)
    cov, Yv = ChainCov.from_csr(A.rowptr, A.colidx, A.vals, nchains, max_steps=its, lowrank=lowrank), Y0.clone()
    mg.sample_chains(b, Yv, its, seeds, cov=cov)
    assert torch.equal(Ys, steps[-1]) and torch.equal(Yv, steps[-1])
    assert cs.count() == cs_loop.count() == (its, its * nchains)
    for got, want in zip(cs.fields(), cs_loop.fields()):
        assert torch.equal(got, want)
    for q in range(2):
        assert np.array_equal(cs.trace(q), cs_loop.trace(q)) and np.isfinite(cs.trace(q)).all()
    assert cov.count() == its and np.array_equal(cov.errors(), cov_loop.errors()) and np.isfinite(cov.errors()).all()


@pytest.mark.parametrize("form", ["rows", "wide"])
def test_side_stream(form, delay, streams):  # noqa: F811
    """a first call on a non-default stream gives the default-stream bits; a second call with the same sizes and seeds is
    ordered behind the stream's queue and does not synchronise the host (the slow-producer pattern)"""
    import torch

    A, mg_side = _small(form)
    _, mg_twin = _small(form)
    n, nchains = A.n, 8
    rng = np.random.default_rng(4)
    b, Y0 = W.dev(rng.standard_normal(n)), W.dev(rng.standard_normal((n, nchains)))
    seeds = W.SEEDS[:nchains]
    want = Y0.clone()
    mg_twin.sample_chains(b, want, 2, seeds, counter0=2)
    torch.cuda.synchronize()
    st, third = streams
    first = Y0.clone()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        mg_side.sample_chains(b, first, 2, seeds, counter0=2)
    st.synchronize()
    assert torch.equal(first, want)
    b_side, y_side = torch.full_like(b, float("nan")), torch.full_like(Y0, float("nan"))
    torch.cuda.synchronize()
    with W.no_collection(), torch.cuda.stream(st):
        delay()
        b_side.copy_(b)
        y_side.copy_(Y0)
        with torch.cuda.stream(third):
            seen_queued = b_side.clone()
        mg_side.sample_chains(b_side, y_side, 2, seeds, counter0=2)
        with torch.cuda.stream(third):
            seen_returned = b_side.clone()
    torch.cuda.synchronize()
    assert bool(torch.isnan(seen_queued).all()), "delay too short: the poison was gone once the producer was queued"
    assert bool(torch.isnan(seen_returned).all()), "delay too short: the poison was gone when the call returned (or the call synchronises the host)"
    assert torch.equal(b_side, b)
    assert torch.equal(y_side, want)


@pytest.mark.parametrize("literal", [False, True])
@pytest.mark.parametrize("coarse,sweep", [("cholsampler", 1), ("gibbs", 3)])
@pytest.mark.parametrize("form", ["rows", "wide"])
def test_algorithmic_bytes(form, coarse, sweep, literal):
    """the update's share of the byte model = the formula in the comment of pmg_mgmc_get_algorithmic_bytes_chains, evaluated here
    from the sizes level_lowrank_sizes reports"""
    A, ops, ps = W.hierarchy_17()
    k, nu, coarse_its = 5, 2, 3
    kw = dict(coarse=coarse, sweep=sweep, nu=nu, coarse_its=coarse_its)
    mg = W.make_mgmc(ops, ps, W.observations_17(form, k, 9), **kw)
    plain = W.make_mgmc(ops, ps, None, **kw)
    mg.set_correction_form(literal)
    plain.set_correction_form(literal)
    for C in (1, 7, 64):
        tot, per = mg.algorithmic_bytes_chains(C)
        tot0, per0 = plain.algorithmic_bytes_chains(C)
        want = W.lowrank_chain_bytes(mg, ops, k, C, coarse, nu, 2 if sweep == 3 else 1, coarse_its, literal)
        assert want > 0 and tot - tot0 == want, (C, tot - tot0, want)
        assert np.isclose(per.sum(), tot, rtol=1e-14) and (per >= per0).all()


# smallest multiple of 10 steps (one V-cycle each) at which both bounds of the statistical test hold on an MI355X: measured
# 0.99 (posterior) and 4.70 (prior) Monte-Carlo errors after 10 cycles, 0.98 / 4.72 after 20 and 30, 1.02 / 4.73 after 40
MATLRC_STEPS = 10


def test_ex6_shape_posterior_covariance_matlrc_mgmc():
    """The operator, observations, seeds, Monte-Carlo error and both bounds of test_ex6_shape_posterior_covariance
    (tests/test_gpu_lowrank_chains.py): 1000 chains from zero with MGMC on the MATLRC hierarchy (coarse_max = 100), ONE cycle per
    step.  The covariance error against (A + B S B^T)^-1 falls below twice the Monte-Carlo error after MATLRC_STEPS cycles --
    the Woodbury route on the prior MGMC chains needs 200 (10 steps of 20 cycles) -- and stays above three times that error
    against the prior A^-1."""
    import torch

    from parmgmc_amd.unstructured import build_hierarchy

    A, B, S, post, prior, seeds, mc_err = W.ex6_posterior()
    ops, ps = build_hierarchy(A.scipy().tocsr(), coarse_max=100)
    mg = W.make_mgmc(ops, ps, (B, S))
    n, nchains = A.n, len(seeds)
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    Y = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    assert mg.sample_chains(b, Y, MATLRC_STEPS, seeds) == MATLRC_STEPS
    e_post, e_prior = W.cov_err(Y, post, post), W.cov_err(Y, prior, post)
    print(f"MATLRC MGMC, {MATLRC_STEPS} cycles: error against the posterior {e_post:.4f}, against the prior {e_prior:.4f}, Monte-Carlo error {mc_err:.4f}")
    assert e_post < 2.0 * mc_err, (e_post, mc_err)
    assert e_prior > 3.0 * mc_err, (e_prior, mc_err)
