"""Column c of a chains call equals the single-chain call, bit for bit (torch.equal), at the chain counts of
tests/woodbury_cases.py that the suite had not launched -- lane splits LPRL = 1 (C = 2) and 4 (C = 9 .. 16), the exact powers of
two, one chunk with dead lanes and full, the chunk edges 64 and 128 | 129 -- through the paths that pick the compact and the
one-block kernels of kernels_lrc_chains.hip (tests/test_gpu_woodbury_term.py has the dense Woodbury form):

  MCSOR.set_lowrank + sample_chains / apply_chains on 17 x 17 x 9: the compact form (pmg_lrc_post_chains: always the three
  launches, lrc_btx_chains_kernel<4, true, LPRL> on one block of support rows here), wide observations and PMG_LRC_DENSE=1
  (<16, false, LPRL>); the colour sweeps give the SELL chain kernels of kernels_chains.hip the same lpr_log2.

  MGMC.sample_chains with one shared and one right-hand side per chain (pmg_mgmc_sample_chains_rhs) on hierarchies with a
  low-rank update, both correction forms.  mg_vcycle_chains (pmg_mgmc_chains.c) runs a level's sweeps through
  pmg_mcsor_sweeps_lowrank_chains and its residual through pmg_mcsor_residual_chains; their repair
  (pmg_lrc_post_restore_chains) and residual term (pmg_lrc_residual_sub_chains) meet in lrc_btx_update_chains (pmg_lrc.c),
  which picks the kernel -- the rule pmg_lrc_chains_fused reports to the byte model of pmg_mgmc_chains.c:
  compact with 0 < support <= 1024 rows: lrc_small_chains_kernel<LPRL>, one workgroup per chunk of 64 chains; compact with
  more: lrc_btx_chains_kernel<4, true, LPRL> + reduction + update; dense: lrc_btx_chains_kernel<16, false, LPRL>.  The tests
  assert the support sizes that decide it: the 17 x 17 x 9 hierarchy with ball observations is one-block on its fine level, its
  coarsest and one between (dense where the coarsened balls pass a quarter of a level's rows); the refined L-shape has several
  blocks on its fine level and, with three balls, one block on a level below (with five: two blocks there, dense below)."""
import numpy as np
import pytest

import lrc_chain_workloads as L
import woodbury_cases as W
from lrc_chain_workloads import config4  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
MAXC = max(W.CHAINS)
SEEDS = W.chain_seeds(MAXC)
MGMC_COUNTS = [2, 16, 64, 129]
assert set(MGMC_COUNTS) <= set(W.CHAINS) and {W.CHAIN_TABLE[C][0] for C in MGMC_COUNTS} == {1, 4, 6}


# ---- MCSOR with a low-rank update ------------------------------------------------------------------------------------------------
_MCSOR = {}


def _mcsor(monkeypatch, form, k):
    """the sampler, b, MAXC start columns and the single-chain results (noisy symmetric sweeps at omega = 1.3; the
    deterministic apply) of every column, once per (form, k)"""
    import torch

    import oracle as O
    from parmgmc_amd import MCSOR, SOR_SYMMETRIC_SWEEP

    if (form, k) not in _MCSOR:
        if form == "dense_env":
            monkeypatch.setenv("PMG_LRC_DENSE", "1")  # read when the update is built
        else:
            monkeypatch.delenv("PMG_LRC_DENSE", raising=False)
        A = O.shifted_laplace(*L.GRID17, 2.0)
        mc = MCSOR(A.rowptr, A.colidx, A.vals).setup()
        mc.set_lowrank(*L.observations_17("rows" if form == "dense_env" else form, k, 10 * k))
        mc.set_omega(1.3)
        mc.set_sweep_type(SOR_SYMMETRIC_SWEEP)
        rng = np.random.default_rng(k)
        b, Y0 = L.dev(rng.standard_normal(A.n)), L.dev(rng.standard_normal((A.n, MAXC)))
        sampled, applied = [], []
        for c in range(MAXC):
            y = Y0[:, c].contiguous()
            assert mc.sample(b, y, 2, SEEDS[c], counter0=5) == 9  # two noise draws per symmetric sweep
            sampled.append(y)
            y = Y0[:, c].contiguous()
            mc.apply(b, y)
            applied.append(y)
        _MCSOR[(form, k)] = mc, b, b.clone(), Y0, torch.stack(sampled, 1), torch.stack(applied, 1)
    return _MCSOR[(form, k)]


@pytest.mark.parametrize("nchains", W.CHAINS)
@pytest.mark.parametrize("k", [3, 5, 64])
@pytest.mark.parametrize("form", ["rows", "wide", "dense_env"])
def test_mcsor_lowrank_chains(monkeypatch, form, k, nchains):
    import torch

    mc, b, b_keep, Y0, sampled, applied = _mcsor(monkeypatch, form, k)
    Y = Y0[:, :nchains].clone()
    assert mc.sample_chains(b, Y, 2, SEEDS[:nchains], counter0=5) == 9
    for c in range(nchains):
        assert torch.equal(Y[:, c], sampled[:, c]), ("sample", c)
    Y = Y0[:, :nchains].clone()
    mc.apply_chains(b, Y)
    for c in range(nchains):
        assert torch.equal(Y[:, c], applied[:, c]), ("apply", c)
    assert torch.equal(b, b_keep), "b changed"
    assert not torch.equal(sampled[:, 0], applied[:, 0]) and not torch.equal(sampled[:, 0], sampled[:, 1])


# ---- MGMC with a low-rank update -------------------------------------------------------------------------------------------------
_MGMC = {}
FORMS = [(False, False), (False, True), (True, False), (True, True)]  # (literal correction form, one right-hand side per chain)


def _single_columns(mg, n, maxc, seed):
    """b (shared), Bp (one per chain), Y0 and the single-chain results of every column in every form"""
    import torch

    rng = np.random.default_rng(seed)
    b, Bp, Y0 = L.dev(rng.standard_normal(n)), L.dev(rng.standard_normal((n, maxc))), L.dev(rng.standard_normal((n, maxc)))
    singles = {}
    for literal, rhs in FORMS:
        mg.set_correction_form(literal)
        cols = []
        for c in range(maxc):
            y = Y0[:, c].contiguous()
            assert mg.sample(Bp[:, c].contiguous() if rhs else b, y, 2, SEEDS[c], counter0=3) == 5
            cols.append(y)
        singles[(literal, rhs)] = torch.stack(cols, 1)
    mg.set_correction_form(False)
    return dict(mg=mg, n=n, b=b, Bp=Bp, Y0=Y0, singles=singles)


def _compare_mgmc(s, nchains):
    import torch

    mg = s["mg"]
    for literal, rhs in FORMS:
        mg.set_correction_form(literal)
        rhs_in = s["Bp"][:, :nchains].contiguous() if rhs else s["b"]
        keep = rhs_in.clone()
        Y = s["Y0"][:, :nchains].clone()
        assert mg.sample_chains(rhs_in, Y, 2, SEEDS[:nchains], counter0=3) == 5
        assert torch.equal(rhs_in, keep), "the right-hand side changed"
        want = s["singles"][(literal, rhs)]
        for c in range(nchains):
            assert torch.equal(Y[:, c], want[:, c]), (literal, rhs, c)
    mg.set_correction_form(False)
    assert not torch.equal(s["singles"][FORMS[0]][:, 0], s["singles"][FORMS[1]][:, 0])


def _grid17(form, k):
    if ("grid17", form, k) not in _MGMC:
        A, ops, ps = L.hierarchy_17()
        mg = L.make_mgmc(ops, ps, L.observations_17(form, k, 10 * k), "gibbs", 1.0, True, 3)
        sizes = [L.level_lowrank_sizes(mg, ops, l) for l in range(len(ops))]
        assert all(kk == k for kk, _, _ in sizes)
        if form == "rows":
            # the fine level, the Gibbs coarsest one and one between: compact, one block of support rows, lrc_small_chains_kernel;
            # where the coarsened balls cover more than a quarter of a level's rows it is dense (one block of 4096 rows)
            small = [not dense and 0 < rows <= L.ROWS_PER_BLOCK for _, rows, dense in sizes]
            assert small[-1] and small[0] and sum(small) >= 3, sizes
            assert all(sm or (dense and rows <= L.DENSE_ROWS_PER_BLOCK) for sm, (_, rows, dense) in zip(small, sizes)), sizes
        else:  # every column on a third of the rows: the dense form on the fine level, lrc_btx_chains_kernel<16, false, LPRL>
            assert sizes[-1][2] and A.n <= L.DENSE_ROWS_PER_BLOCK, sizes
        _MGMC[("grid17", form, k)] = _single_columns(mg, A.n, MAXC, k)
    return _MGMC[("grid17", form, k)]


@pytest.mark.parametrize("nchains", MGMC_COUNTS)
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("form", ["rows", "wide"])
def test_mgmc_lowrank_chains_grid17(form, k, nchains):
    _compare_mgmc(_grid17(form, k), nchains)


def _lshape3(k):
    if ("lshape3", k) not in _MGMC:
        from parmgmc_amd import COLORING_ITERATED

        A, ops, ps, B, S = L.lshape3(k)
        mg = L.make_mgmc(ops, ps, (B, S), "cholsampler", coloring=COLORING_ITERATED)
        top = len(ops) - 1
        sizes = [L.level_lowrank_sizes(mg, ops, l) for l in range(1, top + 1)]  # above the exact coarse sampler
        # the fine level: compact, more than two blocks of 1024 support rows -- lrc_btx_chains_kernel<4, true, LPRL>
        assert not sizes[-1][2] and sizes[-1][1] > 2 * L.ROWS_PER_BLOCK, sizes
        if k == 3:  # a level below: compact, one block -- lrc_small_chains_kernel<LPRL>
            assert any(not dense and 0 < rows <= L.ROWS_PER_BLOCK for _, rows, dense in sizes[:-1]), sizes
        else:  # five balls: the level below is compact with two blocks as well, the next one dense
            assert sum(not dense and rows > L.ROWS_PER_BLOCK for _, rows, dense in sizes) >= 2 and any(dense for _, _, dense in sizes), sizes
        _MGMC[("lshape3", k)] = _single_columns(mg, A.shape[0], MAXC, 100 + k)
    return _MGMC[("lshape3", k)]


@pytest.mark.parametrize("nchains", MGMC_COUNTS)
@pytest.mark.parametrize("k", [3, 5])
def test_mgmc_lowrank_chains_lshape3(k, nchains):
    _compare_mgmc(_lshape3(k), nchains)


@pytest.mark.parametrize("nchains", [2, 16])
def test_mgmc_lowrank_chains_config4(config4, nchains):  # noqa: F811
    """BASELINE config 4 (377 089 rows, 11 blocks of support rows on the fine level) at the two lane splits that were new"""
    from parmgmc_amd import COLORING_ITERATED

    A, ops, ps, B, S, cache = config4
    if "lane_splits" not in cache:
        mg = L.make_mgmc(ops, ps, (B, S), "cholsampler", coloring=COLORING_ITERATED)
        top = len(ops) - 1
        sizes = [L.level_lowrank_sizes(mg, ops, l) for l in range(1, top + 1)]
        assert not sizes[-1][2] and sizes[-1][1] > 10 * L.ROWS_PER_BLOCK, sizes
        assert any(not dense and 0 < rows <= L.ROWS_PER_BLOCK for _, rows, dense in sizes[:-1]), sizes
        cache["lane_splits"] = _single_columns(mg, A.shape[0], 16, 4)
    _compare_mgmc(cache["lane_splits"], nchains)


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _MCSOR.clear()
    _MGMC.clear()
