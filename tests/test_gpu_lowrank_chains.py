"""Posterior sampling on many chains per call: MCSOR chains on an operator with a low-rank (MATLRC) update, the per-chain
right-hand-side entry points of MCSOR and MGMC, and PCWOODBURY on C chains.  Column c of every chains call equals, bit for
bit (torch.equal), the single-chain call on that column alone with seed = seeds[c] (and b = B[:, c] for the per-chain
right-hand sides).  Last, an ex6-shaped covariance check of both posterior chain samplers over 1000 chains."""
from pathlib import Path

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
SEEDS = [0xBEEF + 1009 * c for c in range(80)]
SWEEP_CONFIGS = [(1.0, True), (1.0, False), (1.3, True)]  # (omega, scaled)
LSHAPE_BALLS = [(0.5, 0.5), (1.5, 0.5), (0.5, 1.5)]  # inside the L: [0, 2]^2 without [1, 2]^2


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def grid_balls(grid, centres, radius):
    """ball indicators on the unit-cube grid, natural order with x fastest"""
    nx, ny, nz = grid
    X, Y, Z = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny), np.linspace(0, 1, nz), indexing="ij")
    pts = np.stack([X.ravel(order="F"), Y.ravel(order="F"), Z.ravel(order="F")], 1)
    return [((pts - np.asarray(c)) ** 2).sum(1) < radius * radius for c in centres]


def observations_17(form, k, seed):
    """B (n x k) and S on the 17 x 17 x 9 grid.  rows / dense_env: the k columns are random weights on two small balls (a
    support far below a quarter of the rows: the row-compact form unless PMG_LRC_DENSE is set); wide: every column on a
    third of the rows (the dense form)."""
    grid = (17, 17, 9)
    n = int(np.prod(grid))
    rng = np.random.default_rng(seed)
    B = np.zeros((n, k))
    if form == "wide":
        for j in range(k):
            idx = rng.choice(n, size=n // 3, replace=False)
            B[idx, j] = rng.uniform(0.5, 1.5, len(idx)) / len(idx)
    else:
        balls = grid_balls(grid, [(0.3, 0.3, 0.4), (0.7, 0.6, 0.6)], 0.16)
        for j in range(k):
            inside = balls[j % 2]
            B[inside, j] = rng.uniform(0.5, 1.5, inside.sum()) / inside.sum()
    return B, rng.uniform(20.0, 90.0, k)


def _compare_mcsor(mc, n, nchains, rng, sweep_types=None, configs=SWEEP_CONFIGS, its=3):
    import torch

    from parmgmc_amd import SOR_BACKWARD_SWEEP, SOR_FORWARD_SWEEP, SOR_SYMMETRIC_SWEEP

    b = dev(rng.standard_normal(n))
    b_keep = b.clone()
    Y0 = dev(rng.standard_normal((n, nchains)))
    seeds = SEEDS[:nchains]
    for om, scaled in configs:
        mc.set_omega(om)
        for t in sweep_types or (SOR_FORWARD_SWEEP, SOR_BACKWARD_SWEEP, SOR_SYMMETRIC_SWEEP):
            mc.set_sweep_type(t)
            Y = Y0.clone()
            ctr = mc.sample_chains(b, Y, its, seeds, counter0=5, scaled=scaled)
            assert torch.equal(b, b_keep), "b changed"
            for c in range(nchains):
                y = Y0[:, c].contiguous()
                assert mc.sample(b, y, its, seeds[c], counter0=5, scaled=scaled) == ctr
                assert torch.equal(Y[:, c], y), (om, scaled, t, c)
            Y = Y0.clone()
            mc.apply_chains(b, Y)
            assert torch.equal(b, b_keep), "b changed by apply_chains"
            for c in range(nchains):
                y = Y0[:, c].contiguous()
                mc.apply(b, y)
                assert torch.equal(Y[:, c], y), ("apply", om, t, c)


@pytest.mark.parametrize("nchains", [1, 3, 32, 65])
@pytest.mark.parametrize("k", [1, 3, 17, 64])
@pytest.mark.parametrize("form", ["rows", "wide", "dense_env"])
def test_mcsor_lowrank_chains_small(monkeypatch, form, k, nchains):
    from parmgmc_amd import MCSOR

    if form == "dense_env":
        monkeypatch.setenv("PMG_LRC_DENSE", "1")  # read when the update is built
    else:
        monkeypatch.delenv("PMG_LRC_DENSE", raising=False)
    A = O.shifted_laplace(17, 17, 9, 2.0)
    mc = MCSOR(A.rowptr, A.colidx, A.vals).setup()
    mc.set_lowrank(*observations_17(form, k, 10 * k + nchains))
    _compare_mcsor(mc, A.n, nchains, np.random.default_rng(k * nchains))


@pytest.fixture(scope="module")
def config4():
    """BASELINE config 4 (bench.py's unstructured_secondary): lshape.msh refined 5 times, P1 kappa^2 M + K, the aggregation
    hierarchy with coarse_max = 2000; plus three ball observations of ~3700 vertices each"""
    from parmgmc_amd.unstructured import assemble_p1, ball_observations, build_hierarchy, read_gmsh41_triangles, refine_uniform

    xy, tris = read_gmsh41_triangles(GOLD / "lshape.msh")
    for _ in range(5):
        xy, tris = refine_uniform(xy, tris)
    A = assemble_p1(xy, tris, 1.0)
    ops, ps = build_hierarchy(A, coarse_max=2000)
    B = ball_observations(xy, LSHAPE_BALLS, 0.1)
    assert ((B > 0).sum(0) > 3000).all()
    return A, ops, ps, B, np.array([40.0, 60.0, 80.0])


@pytest.mark.parametrize("nchains", [1, 8, 32])
def test_mcsor_lowrank_chains_config4(config4, nchains):
    """several 1024-row blocks of support rows"""
    from parmgmc_amd import COLORING_ITERATED, MCSOR, SOR_FORWARD_SWEEP, SOR_SYMMETRIC_SWEEP

    A, _, _, B, S = config4
    mc = MCSOR(A.indptr, A.indices, A.data, COLORING_ITERATED).setup()
    mc.set_lowrank(B, S)
    _compare_mcsor(mc, A.shape[0], nchains, np.random.default_rng(nchains), (SOR_FORWARD_SWEEP, SOR_SYMMETRIC_SWEEP), [(1.0, True)], its=2)


@pytest.mark.parametrize("lowrank", [False, True])
def test_mcsor_chains_per_chain_rhs(config4, lowrank):
    import torch

    from parmgmc_amd import COLORING_ITERATED, MCSOR, SOR_SYMMETRIC_SWEEP

    A, _, _, B, S = config4
    n, nchains = A.shape[0], 8
    mc = MCSOR(A.indptr, A.indices, A.data, COLORING_ITERATED).setup()
    if lowrank:
        mc.set_lowrank(B, S)
    mc.set_sweep_type(SOR_SYMMETRIC_SWEEP)
    rng = np.random.default_rng(3)
    Bp = dev(rng.standard_normal((n, nchains)))
    B_keep = Bp.clone()
    Y0 = dev(rng.standard_normal((n, nchains)))
    Y = Y0.clone()
    ctr = mc.sample_chains(Bp, Y, 2, SEEDS[:nchains], counter0=4)
    assert torch.equal(Bp, B_keep)
    for c in range(nchains):
        y = Y0[:, c].contiguous()
        assert mc.sample(Bp[:, c].contiguous(), y, 2, SEEDS[c], counter0=4) == ctr
        assert torch.equal(Y[:, c], y), c


def _mgmc(ops, ps, coarse):
    from parmgmc_amd import COLORING_ITERATED, MGMC

    mg = MGMC.from_hierarchy(ops, ps)
    mg.set_coloring(COLORING_ITERATED)
    mg.set_smoother(True, 1.0, 1, 1)
    mg.set_coarse(coarse, 1)
    return mg.setup()


@pytest.mark.parametrize("coarse", ["cholsampler", "gibbs"])
def test_mgmc_chains_per_chain_rhs(config4, coarse):
    import torch

    _, ops, ps, _, _ = config4
    mg = _mgmc(ops, ps, coarse)
    n, rng = mg.n, np.random.default_rng(5)
    for nchains in (1, 8):
        for literal in (False, True):
            for guesszero in (False, True):
                mg.set_correction_form(literal)
                Bp = dev(rng.standard_normal((n, nchains)))
                B_keep = Bp.clone()
                Y0 = dev(rng.standard_normal((n, nchains)))
                Y = Y0.clone()
                assert mg.sample_chains(Bp, Y, 2, SEEDS[:nchains], counter0=3, guesszero=guesszero) == 5
                assert torch.equal(Bp, B_keep)
                for c in range(nchains):
                    y = Y0[:, c].contiguous()
                    mg.sample(Bp[:, c].contiguous(), y, 2, SEEDS[c], counter0=3, guesszero=guesszero)
                    assert torch.equal(Y[:, c], y), (nchains, literal, guesszero, c)


def _jacobi_solve(A):
    """a deterministic stand-in solver for the Woodbury set-up: x = D^-1 b (bit identity does not need a good one)"""
    dinv = dev(1.0 / A.diagonal())

    def solve(b, x):
        x.copy_(b * dinv)

    return solve


def _woodbury_mgmc(A, mg, B, S, state):
    """WoodburySampler on the MGMC prior: one V-cycle per step; state["seed"] = the single-chain sampler's seed, state["seeds"]
    the chains'"""
    from parmgmc_amd.wrappers import WoodburySampler

    return WoodburySampler(B, S, _jacobi_solve(A), lambda w, y, ctr: mg.sample(w, y, 1, state["seed"], counter0=ctr),
                           sample_chains=lambda W, Y, ctr: mg.sample_chains(W, Y, 1, state["seeds"], counter0=ctr))


def test_woodbury_chains_steps(config4):
    import torch

    from parmgmc_amd.capi import check, lib
    from parmgmc_amd.wrappers import _ptr, _seeds, _stream

    A, ops, ps, B, S = config4
    mg = _mgmc(ops, ps, "cholsampler")
    wb = _woodbury_mgmc(A, mg, B, S, {})
    n, rng = A.shape[0], np.random.default_rng(6)
    for nchains in (1, 3, 65):
        seeds = _seeds(SEEDS[:nchains], nchains)
        b = dev(rng.standard_normal(n))
        W = torch.full((n, nchains), np.nan, dtype=torch.float64, device="cuda")
        check(lib.pmg_woodbury_noisy_rhs_chains(wb._h, nchains, seeds.ctypes.data, 7, _ptr(b), _ptr(W), _stream()))
        Y0 = dev(rng.standard_normal((n, nchains)))
        Y = Y0.clone()
        check(lib.pmg_woodbury_correct_chains(wb._h, nchains, _ptr(Y), _stream()))
        for c in range(nchains):
            w = torch.empty(n, dtype=torch.float64, device="cuda")
            check(lib.pmg_woodbury_noisy_rhs(wb._h, _ptr(b), _ptr(w), int(seeds[c]), 7, _stream()))
            assert torch.equal(W[:, c], w), ("noisy_rhs", nchains, c)
            y = Y0[:, c].contiguous()
            check(lib.pmg_woodbury_correct(wb._h, _ptr(y), _stream()))
            assert torch.equal(Y[:, c], y), ("correct", nchains, c)


def test_woodbury_mgmc_run_chains(config4):
    import torch

    A, ops, ps, B, S = config4
    mg = _mgmc(ops, ps, "cholsampler")
    state = {}
    wb = _woodbury_mgmc(A, mg, B, S, state)
    n, rng = A.shape[0], np.random.default_rng(7)
    b = dev(rng.standard_normal(n))
    for nchains in (1, 8, 32):
        Y0 = dev(rng.standard_normal((n, nchains)))
        Y = Y0.clone()
        state["seeds"] = SEEDS[:nchains]
        assert wb.run_chains(b, Y, 3, SEEDS[:nchains], counter0=2) == 5
        for c in range(nchains):
            y = Y0[:, c].contiguous()
            state["seed"] = SEEDS[c]
            wb.run(b, y, 3, SEEDS[c], counter0=2)
            assert torch.equal(Y[:, c], y), (nchains, c)
    # resume: its = 2 twice == its = 4 once; equal seeds on equal columns give equal columns
    seeds = list(SEEDS[:8])
    seeds[5] = seeds[2]
    state["seeds"] = seeds
    Y0 = dev(rng.standard_normal((n, 8)))
    Y0[:, 5] = Y0[:, 2]
    Ya, Yb = Y0.clone(), Y0.clone()
    c1 = wb.run_chains(b, Ya, 2, seeds, counter0=11)
    assert wb.run_chains(b, Ya, 2, seeds, counter0=c1) == 15
    wb.run_chains(b, Yb, 4, seeds, counter0=11)
    assert torch.equal(Ya, Yb)
    assert torch.equal(Ya[:, 5], Ya[:, 2]) and not torch.equal(Ya[:, 4], Ya[:, 2])


def test_ex6_shape_posterior_covariance():
    """examples/ex6.c with three observations: 1000 chains from zero on the ~1000-row operator, for the MATLRC Gibbs chains
    (mcgibbs, forward) and for Woodbury on the MGMC chains.  The covariance error against (A + B S B^T)^-1 falls below twice
    the Monte-Carlo error of 1000 samples (0.28 here); against the prior A^-1 it stays above three times that (the two
    covariances are 1.29 apart in that norm)."""
    import torch

    from parmgmc_amd import MCSOR, MGMC
    from parmgmc_amd.wrappers import WoodburySampler
    from parmgmc_amd.unstructured import build_hierarchy

    A = O.ex6_matrix(32, 1e-2)
    n, nchains = A.n, 1000
    Ad = A.scipy().toarray()
    side = int(round(np.sqrt(n)))
    X, Yg = np.meshgrid(np.linspace(0, 1, side), np.linspace(0, 1, side), indexing="ij")
    pts = np.stack([X.ravel(order="F"), Yg.ravel(order="F")], 1)
    B = np.zeros((n, 3))
    for j, ctr in enumerate([(0.25, 0.3), (0.7, 0.5), (0.4, 0.8)]):
        inside = ((pts - np.asarray(ctr)) ** 2).sum(1) < 0.2**2
        B[inside, j] = 1.0 / inside.sum()
    S = np.array([1e4, 2e4, 5e4])
    post = np.linalg.inv(Ad + B @ np.diag(S) @ B.T)
    prior = np.linalg.inv(Ad)
    seeds = [0x5EED0000 + 7919 * c for c in range(nchains)]

    def cov_err(Ys, Sigma):
        """||C_N - Sigma||_F / ||(A + B S B^T)^-1||_F for the sample covariance C_N over the chains"""
        X = Ys.T.contiguous().cpu().numpy()
        Cn = np.cov(X, rowvar=False)
        return np.linalg.norm(Cn - Sigma) / np.linalg.norm(post)

    fro = np.linalg.norm(post)
    mc_err = np.sqrt((fro**2 + np.trace(post) ** 2) / (nchains - 1)) / fro
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    # MATLRC Gibbs chains
    mc = MCSOR(A.rowptr, A.colidx, A.vals).setup()
    mc.set_lowrank(B, S)
    Y = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    mc.sample_chains(b, Y, 800, seeds)
    e_post, e_prior = cov_err(Y, post), cov_err(Y, prior)
    assert e_post < 2.0 * mc_err, (e_post, mc_err)
    assert e_prior > 3.0 * mc_err, (e_prior, mc_err)
    # Woodbury on the MGMC chains (exact solver for the set-up).  PCWOODBURY samples the posterior exactly when its prior sampler
    # is exact; a Markov prior sampler leaves its error propagation on the huge A^-1 B S B^T A^-1 of this nearly singular
    # operator (one MGMC cycle per step: error 400, five: 27).  Twenty cycles per step bring it to the Monte-Carlo error.
    ops, ps = build_hierarchy(A.scipy().tocsr(), coarse_max=100)
    mg = MGMC.from_hierarchy(ops, ps)
    mg.set_smoother(True, 1.0, 1, 1)
    mg.setup()
    Ainv = dev(prior)

    def solve(rhs, x):
        x.copy_(Ainv @ rhs)

    cycles = 20
    wb = WoodburySampler(B, S, solve, lambda w, y, ctr: None, sample_chains=lambda W, Yc, ctr: mg.sample_chains(W, Yc, cycles, seeds, counter0=ctr * cycles))
    Y = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    wb.run_chains(b, Y, 10, seeds)
    e_post, e_prior = cov_err(Y, post), cov_err(Y, prior)
    assert e_post < 2.0 * mc_err, (e_post, mc_err)
    assert e_prior > 3.0 * mc_err, (e_prior, mc_err)
