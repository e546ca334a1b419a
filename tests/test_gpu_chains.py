"""Many chains per call (pmg_mcsor_apply_chains / pmg_mcsor_sample_chains / pmg_mgmc_sample_chains): column c of every
chains call equals, bit for bit (torch.equal), the single-chain call on that column alone with seed = seeds[c]."""
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import oracle as O

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def random_spd(n, density, seed):
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=density, random_state=rng, format="csr")
    M = M + M.T
    M = M + sp.diags(np.abs(M).sum(axis=1).A1 + 1.0)
    return O.CSR.from_scipy(M)


def small_cases():
    yield "lap9x9", O.shifted_laplace(9, 9, 1, 10.0)
    yield "lap6x5x4", O.shifted_laplace(6, 5, 4, 2.0)
    yield "galerkin27", O.CSR.from_scipy(O.galerkin(O.shifted_laplace(9, 9, 9, 1.0).scipy(), O.q1_interp(5, 5, 5)))
    yield "random200", random_spd(200, 0.03, 1)


@pytest.fixture(scope="module")
def config4():
    """BASELINE config 4 as bench.py's unstructured_secondary builds it: lshape.msh refined 5 times, P1 kappa^2 M + K, the
    aggregation hierarchy with coarse_max = 2000"""
    from parmgmc_amd.unstructured import assemble_p1, build_hierarchy, read_gmsh41_triangles, refine_uniform

    xy, tris = read_gmsh41_triangles(GOLD / "lshape.msh")
    for _ in range(5):
        xy, tris = refine_uniform(xy, tris)
    A = assemble_p1(xy, tris, 1.0)
    ops, ps = build_hierarchy(A, coarse_max=2000)
    assert [len(o[0]) - 1 for o in ops] == [1549, 6033, 23809, 94593, 377089]
    return A, ops, ps


SEEDS = [0xCAFE + 977 * c for c in range(80)]
SWEEP_CONFIGS = [(1.0, True), (1.0, False), (1.3, True)]  # (omega, scaled)


def _mcsor_compare(mc, n, nchains, rng):
    import torch

    from parmgmc_amd import SOR_BACKWARD_SWEEP, SOR_FORWARD_SWEEP, SOR_SYMMETRIC_SWEEP

    b = dev(rng.standard_normal(n))
    Y0 = dev(rng.standard_normal((n, nchains)))
    seeds = SEEDS[:nchains]
    for om, scaled in SWEEP_CONFIGS:
        mc.set_omega(om)
        for t in (SOR_FORWARD_SWEEP, SOR_BACKWARD_SWEEP, SOR_SYMMETRIC_SWEEP):
            mc.set_sweep_type(t)
            Y = Y0.clone()
            ctr = mc.sample_chains(b, Y, 3, seeds, counter0=5, scaled=scaled)
            for c in range(nchains):
                y = Y0[:, c].contiguous()
                ctr1 = mc.sample(b, y, 3, seeds[c], counter0=5, scaled=scaled)
                assert torch.equal(Y[:, c], y), (om, scaled, t, c)
                assert ctr == ctr1
            # the deterministic sweep
            Y = Y0.clone()
            mc.apply_chains(b, Y)
            for c in range(nchains):
                y = Y0[:, c].contiguous()
                mc.apply(b, y)
                assert torch.equal(Y[:, c], y), ("apply", om, t, c)


@pytest.mark.parametrize("nchains", [1, 3, 32, 65])
@pytest.mark.parametrize("name,A", list(small_cases()), ids=[c[0] for c in small_cases()])
def test_mcsor_chains_small(name, A, nchains):
    from parmgmc_amd import MCSOR

    mc = MCSOR(A.rowptr, A.colidx, A.vals).setup()
    _mcsor_compare(mc, A.n, nchains, np.random.default_rng(nchains))


@pytest.mark.parametrize("nchains", [1, 3, 32, 65])
def test_mcsor_chains_config4(config4, nchains):
    from parmgmc_amd import COLORING_ITERATED, MCSOR

    A = config4[0]
    mc = MCSOR(A.indptr, A.indices, A.data, COLORING_ITERATED).setup()
    _mcsor_compare(mc, A.shape[0], nchains, np.random.default_rng(100 + nchains))


def _mgmc(ops, ps, rule, coarse, scaled=True, omega=1.0, sweep_type=1, its=1, coarse_its=1):
    from parmgmc_amd import MGMC

    mg = MGMC.from_hierarchy(ops, ps)
    mg.set_coloring(rule)
    mg.set_smoother(scaled, omega, sweep_type, its)
    mg.set_coarse(coarse, coarse_its)
    return mg.setup()


def _mgmc_compare(mg, n, nchains, literal, guesszero, rng, its=2):
    import torch

    mg.set_correction_form(literal)
    b = dev(rng.standard_normal(n))
    Y0 = dev(rng.standard_normal((n, nchains)))
    seeds = SEEDS[:nchains]
    Y = Y0.clone()
    ctr = mg.sample_chains(b, Y, its, seeds, counter0=3, guesszero=guesszero)
    assert ctr == 3 + its
    assert torch.isfinite(Y).all()
    for c in range(nchains):
        y = Y0[:, c].contiguous()
        mg.sample(b, y, its, seeds[c], counter0=3, guesszero=guesszero)
        assert torch.equal(Y[:, c], y), (nchains, literal, guesszero, c)


@pytest.mark.parametrize("coarse", ["cholsampler", "gibbs"])
@pytest.mark.parametrize("rule", ["greedy", "iterated"])
def test_mgmc_chains_bench_hierarchy(config4, rule, coarse):
    from parmgmc_amd import COLORING_GREEDY, COLORING_ITERATED

    _, ops, ps = config4
    mg = _mgmc(ops, ps, {"greedy": COLORING_GREEDY, "iterated": COLORING_ITERATED}[rule], coarse)
    rng = np.random.default_rng(7)
    for nchains in (1, 8, 32):
        for literal in (False, True):
            for guesszero in (False, True):
                _mgmc_compare(mg, mg.n, nchains, literal, guesszero, rng)


def test_mgmc_chains_symmetric_omega(config4):
    """symmetric sweeps, omega = 1.3, two smoothing and two coarse Gibbs iterations"""
    from parmgmc_amd import COLORING_ITERATED, SOR_SYMMETRIC_SWEEP

    _, ops, ps = config4
    mg = _mgmc(ops, ps, COLORING_ITERATED, "gibbs", True, 1.3, SOR_SYMMETRIC_SWEEP, 2, 2)
    rng = np.random.default_rng(8)
    for literal in (False, True):
        _mgmc_compare(mg, mg.n, 8, literal, False, rng)
    mg = _mgmc(ops, ps, COLORING_ITERATED, "cholsampler", False, 1.0, SOR_SYMMETRIC_SWEEP, 1)  # sorgibbs
    _mgmc_compare(mg, mg.n, 8, False, True, rng)


def test_mgmc_chains_resume_same_seeds_callback(config4):
    import torch

    from parmgmc_amd import COLORING_ITERATED, PMGError

    _, ops, ps = config4
    mg = _mgmc(ops, ps, COLORING_ITERATED, "cholsampler")
    n, rng = mg.n, np.random.default_rng(9)
    b = dev(rng.standard_normal(n))
    Y0 = dev(rng.standard_normal((n, 8)))
    seeds = SEEDS[:8]
    # resume: its = 2 twice with the counter chained == its = 4 once
    Ya, Yb = Y0.clone(), Y0.clone()
    c1 = mg.sample_chains(b, Ya, 2, seeds, counter0=11)
    assert mg.sample_chains(b, Ya, 2, seeds, counter0=c1) == 15
    mg.sample_chains(b, Yb, 4, seeds, counter0=11)
    assert torch.equal(Ya, Yb)
    # equal seeds on two chains started from equal columns give equal columns
    Y = Y0.clone()
    Y[:, 5] = Y[:, 2]
    s2 = list(seeds)
    s2[5] = s2[2]
    mg.sample_chains(b, Y, 2, s2)
    assert torch.equal(Y[:, 5], Y[:, 2]) and not torch.equal(Y[:, 4], Y[:, 2])
    # callback: once per sample with the (n, C) block
    seen = []
    Y = Y0.clone()
    mg.sample_chains(b, Y, 3, seeds, callback=lambda it, Yc: seen.append((it, tuple(Yc.shape), Yc.clone())))
    assert [s[:2] for s in seen] == [(i, (n, 8)) for i in range(3)]
    assert torch.equal(seen[-1][2], Y)
    # a failing callback aborts the loop with its code
    calls = []

    def bad(it, _Y):
        calls.append(it)
        if it == 1:
            raise RuntimeError("stop")

    with pytest.raises(PMGError) as e:
        mg.sample_chains(b, Y0.clone(), 5, seeds, callback=bad)
    assert e.value.code == 77 and calls == [0, 1]


def test_ex6_shape_covariance():
    """examples/ex6.c: 1000 chains on a ~1000-row operator, every chain from zero; the covariance error over the chains
    (pmg_estimate_covariance_errors) falls from 1 at the start to the Monte-Carlo error of 1000 chains"""
    import torch

    from parmgmc_amd import MGMC, estimate_covariance_errors
    from parmgmc_amd.unstructured import build_hierarchy

    A = O.ex6_matrix(32, 1e-2)
    ops, ps = build_hierarchy(A.scipy().tocsr(), coarse_max=100)
    assert len(ops) >= 2
    mg = MGMC.from_hierarchy(ops, ps)
    mg.set_smoother(True, 1.0, 1, 1)  # -gamgmc_mg_levels_pc_mcgibbs_forward
    mg.setup()
    n, nchains, its = A.n, 1000, 40
    seeds = [0x5EED0000 + 7919 * c for c in range(nchains)]
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    Y = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
    mg.sample_chains(b, Y, its, seeds)
    for c in (0, 1, 499, 998, 999):
        y = torch.zeros(n, dtype=torch.float64, device="cuda")
        mg.sample(b, y, its, seeds[c])
        assert torch.equal(Y[:, c], y), c
    # samples [sample][chain][row]: the common start (all zero) and the last sample
    S = np.concatenate([np.zeros((nchains, n)), Y.T.contiguous().cpu().numpy()])
    errs = estimate_covariance_errors(A.rowptr, A.colidx, A.vals, S, nchains)
    Sigma = np.linalg.inv(A.scipy().toarray())
    fro = np.linalg.norm(Sigma)
    mc_err = np.sqrt((fro**2 + np.trace(Sigma) ** 2) / (nchains - 1)) / fro  # E ||C_N - Sigma||_F / ||Sigma||_F of N Gaussian samples
    assert abs(errs[0] - 1.0) < 1e-12
    assert errs[1] < min(2.0 * mc_err, 0.9), (errs, mc_err)
