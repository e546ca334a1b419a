"""The AIJ path on smoothed-aggregation hierarchies and on irregular matrices (tests/aij_workloads.py): rows of hundreds of
entries in the sliced-ELL sweep and residual (kernels_csr.hip), P^T rows of thousands in the CSR transfers
(csr_spmv_rows_kernel and its chain twin), a nearly full coarse matrix in the dense Cholesky sampler -- against the oracle,
bit for bit where the operation order is the oracle's, and with negative controls that prove the comparisons reach the row
tails."""
import zlib
from functools import lru_cache

import numpy as np
import pytest

import aij_workloads as W
import oracle as O

pytestmark = pytest.mark.gpu
GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
LEVELS = {"sa3d25": 3, "sa2d129": 4, "salshape": 3}
RULES = ["greedy", "iterated", "lexlevels"]
ORACLE_RULE = {"greedy": O.coloring_greedy, "iterated": O.coloring_iterated, "lexlevels": O.coloring_lexlevels}
SEEDS = [0xBEEF + 1237 * c for c in range(130)]
TOL = 1e-11


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def level_seed(seed, l):
    return (seed + GOLD * (l + 1)) & M64


def rule_code(rule):
    from parmgmc_amd import COLORING_GREEDY, COLORING_ITERATED, COLORING_LEXLEVELS

    return {"greedy": COLORING_GREEDY, "iterated": COLORING_ITERATED, "lexlevels": COLORING_LEXLEVELS}[rule]


@lru_cache(maxsize=None)
def hier(name):
    return W.hierarchy(name)


@lru_cache(maxsize=None)
def irregular():
    return dict(W.irregular())


@lru_cache(maxsize=None)
def matrix(name) -> O.CSR:
    if name in W.IRREGULAR:
        return irregular()[name]
    h, l = name.split("-L")
    rp, ci, v = hier(h)[0][int(l)]
    return O.CSR(rp, ci, v)


@lru_cache(maxsize=None)
def oracle_colors(name, rule):
    return ORACLE_RULE[rule](matrix(name))


MATRICES = W.IRREGULAR + [f"{h}-L{l}" for h in W.HIERARCHIES for l in range(LEVELS[h])]


# --- structure guards --------------------------------------------------------------------------------------------------------
def test_hierarchies_have_the_wide_rows():
    widest_op = widest_p = widest_pt = 0
    for h in W.HIERARCHIES:
        ops, ps = hier(h)
        assert len(ops) == LEVELS[h]
        widest_op = max([widest_op] + [int(np.diff(o[0]).max()) - 1 for o in ops])  # off-diagonal entries
        widest_p = max([widest_p] + [int(np.diff(p[0]).max()) for p in ps[1:]])
        widest_pt = max([widest_pt] + [int(np.bincount(p[1]).max()) for p in ps[1:]])
    assert widest_op >= 150 and widest_p >= 32 and widest_pt >= 1000, (widest_op, widest_p, widest_pt)
    assert [len(o[0]) - 1 for o in hier("sa3d25")[0]] == [179, 7813, 15625]


def test_irregular_structure():
    from parmgmc_amd import MCSOR

    M = irregular()
    assert np.diff(M["hubs"].rowptr).max() > 3000
    assert oracle_colors("clique", "greedy").max() + 1 >= 40
    assert (M["zeros"].vals == 0).sum() > 1000
    U = M["unsorted"]
    assert any(np.any(np.diff(U.colidx[U.rowptr[r]:U.rowptr[r + 1]]) < 0) for r in range(U.n))
    # isolated: whole slices of width 0 (the first 256 rows are diagonal-only and all in colour 0)
    assert np.all(np.diff(M["isolated"].rowptr)[:256] == 1)
    for n in W.SLICE_EDGE_SIZES:
        assert list(np.bincount(oracle_colors(f"tridiag{n}", "greedy"))) == [(n + 1) // 2, n // 2]
    # scrambled: the breadth-first layout ran, i.e. rows are not ascending inside a colour
    A = M["scrambled"]
    mc = MCSOR(A.rowptr, A.colidx, A.vals).setup()
    lay, col = mc.get_layout(), mc.get_coloring()
    c0 = np.flatnonzero(col == 0)
    assert np.any(np.diff(lay[c0]) < 0)
    mc.destroy()


# --- MCSOR on every matrix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MATRICES)
def test_mcsor_apply_sample_residual(name):
    from parmgmc_amd import MCSOR

    A = matrix(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    b, y0 = rng.standard_normal(A.n), rng.standard_normal(A.n)
    for rule in RULES:
        cols = oracle_colors(name, rule)
        mc = MCSOR(A.rowptr, A.colidx, A.vals, rule_code(rule)).setup()
        assert np.array_equal(mc.get_coloring(), cols), rule
        assert mc.get_num_colors() == cols.max() + 1
        for om in (1.0, 1.3):
            mc.set_omega(om)
            for t in (O.SOR_FORWARD, O.SOR_BACKWARD, O.SOR_SYMMETRIC):
                mc.set_sweep_type(t)
                yd = dev(y0)
                mc.apply(dev(b), yd)
                assert np.array_equal(host(yd), O.mcsor_apply(A, cols, b, y0, om, t)), (rule, om, t)
        for om, scaled in ((1.0, True), (1.3, True), (1.0, False)):
            mc.set_omega(om)
            for t in (O.SOR_FORWARD, O.SOR_BACKWARD, O.SOR_SYMMETRIC):
                mc.set_sweep_type(t)
                yd = dev(y0)
                mc.sample(dev(b), yd, 3, seed=0xCAFE, counter0=5, scaled=scaled)
                want = O.gibbs_samples(A, cols, b, y0, 3, lambda d: O.noise_rows(A.n, 0xCAFE, 5 + d), om, t, scaled)
                assert np.abs(host(yd) - want).max() / np.abs(want).max() < 1e-13, (rule, om, scaled, t)
        r = dev(np.zeros(A.n))
        mc.residual(dev(b), dev(y0), r)
        S = A.scipy()
        Sl = S.astype(np.longdouble)
        want = b.astype(np.longdouble) - Sl @ y0.astype(np.longdouble)
        absum = np.abs(b) + abs(S) @ np.abs(y0)
        assert np.all(np.abs(host(r) - want.astype(np.float64)) <= 4 * np.finfo(np.float64).eps * absum), rule
        mc.destroy()


def _chains_compare(mc, n, nchains, rng):
    """column c of every chains call equals the single-chain call on it, bit for bit"""
    import torch

    b = dev(rng.standard_normal(n))
    Y0 = dev(rng.standard_normal((n, nchains)))
    seeds = SEEDS[:nchains]
    for om, scaled, t in ((1.3, True, O.SOR_SYMMETRIC), (1.0, False, O.SOR_BACKWARD)):
        mc.set_omega(om)
        mc.set_sweep_type(t)
        Y = Y0.clone()
        ctr = mc.sample_chains(b, Y, 3, seeds, counter0=2, scaled=scaled)
        for c in range(nchains):
            y = Y0[:, c].contiguous()
            assert mc.sample(b, y, 3, seeds[c], counter0=2, scaled=scaled) == ctr
            assert torch.equal(Y[:, c], y), (om, scaled, t, c)
        Y = Y0.clone()
        mc.apply_chains(b, Y)
        for c in range(nchains):
            y = Y0[:, c].contiguous()
            mc.apply(b, y)
            assert torch.equal(Y[:, c], y), ("apply", om, t, c)


@pytest.mark.parametrize("nchains", [1, 7, 64, 65, 130])
@pytest.mark.parametrize("name", MATRICES)
def test_mcsor_chains(name, nchains):
    from parmgmc_amd import MCSOR

    A = matrix(name)
    mc = MCSOR(A.rowptr, A.colidx, A.vals).setup()
    _chains_compare(mc, A.n, nchains, np.random.default_rng(nchains))
    mc.destroy()


# --- MGMC on the hierarchies -------------------------------------------------------------------------------------------------
def oracle_mgmc(name, b, y0, its, seed, counter0, guesszero, omega, sweep, coarse, coarse_its=2, P_override=None):
    """the oracle chain of test_gpu_mgmc.py::test_unstructured_hierarchy_lshape: greedy colouring on every level, row-stream
    noise of level_seed(seed, l), 64 draws per sample.  P_override {level: scipy P} replaces the oracle's copy of a P."""
    ops, ps = hier(name)
    L = len(ops)
    csr = [matrix(f"{name}-L{l}") for l in range(L)]
    lv = [dict(A=csr[l].scipy(), P=None if l == 0 else W.as_scipy(ps[l], (csr[l].n, csr[l - 1].n))) for l in range(L)]
    for l, P in (P_override or {}).items():
        lv[l]["P"] = P
    cols = [oracle_colors(f"{name}-L{l}", "greedy") for l in range(L)]
    Lc = O.potrf_lower(csr[0].dense()) if coarse == "cholsampler" else None
    y = np.array(y0, copy=True)
    out = []
    for it in range(its):
        s = counter0 + it
        ctr = {l: 64 * s for l in range(L)}

        def noise(l):
            c = ctr[l]
            ctr[l] += 1
            return O.noise_rows(csr[l].n, level_seed(seed, l), c)

        def smooth(l, rhs, x, leg, its_=1):
            return O.gibbs_samples(csr[l], cols[l], rhs, x, its_, lambda d: noise(l), omega, sweep, True)

        def coarse_fn(rhs):
            if coarse == "cholsampler":
                return O.chol_sample(Lc, rhs, noise(0))
            return smooth(0, rhs, np.zeros(csr[0].n), 0, coarse_its)

        y = O.gamgmc_richardson(lv, b, y, 1, guesszero and it == 0, smooth, coarse_fn)
        out.append(y.copy())
    return out


def make_mgmc(name, omega, sweep, coarse, literal=False, idx_width=32):
    from parmgmc_amd import MGMC

    ops, ps = hier(name)
    mg = MGMC.from_hierarchy(ops, ps, idx_width=idx_width)
    mg.set_smoother(True, omega, sweep, 1)
    mg.set_coarse(coarse, 2 if coarse == "gibbs" else 1)
    mg.set_correction_form(literal)
    return mg.setup()


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("literal", [False, True], ids=["in_place", "correction_form"])
@pytest.mark.parametrize("coarse", ["cholsampler", "gibbs"])
@pytest.mark.parametrize("omega,sweep", [(1.0, O.SOR_FORWARD), (1.1, O.SOR_SYMMETRIC)], ids=["forward", "symmetric1.1"])
@pytest.mark.parametrize("name", W.HIERARCHIES)
def test_mgmc_chain_matches_oracle(name, omega, sweep, coarse, literal):
    n = hier(name)[0][-1][0].shape[0] - 1
    rng = np.random.default_rng(31)
    b, y0 = rng.standard_normal(n), rng.standard_normal(n)
    mg = make_mgmc(name, omega, sweep, coarse, literal)
    seen = []
    yd = dev(y0)
    assert mg.sample(dev(b), yd, 3, seed=0xD00D, counter0=1, callback=lambda it, y: seen.append(host(y).copy())) == 4
    want = oracle_mgmc(name, b, y0, 3, 0xD00D, 1, False, omega, sweep, coarse)
    for s, (got, w) in enumerate(zip(seen, want)):
        assert rel(got, w) < TOL, s
    assert np.array_equal(host(yd), seen[-1])
    mg.destroy()


@pytest.mark.parametrize("name", W.HIERARCHIES)
def test_mgmc_guesszero_matches_oracle(name):
    n = hier(name)[0][-1][0].shape[0] - 1
    b = np.random.default_rng(32).standard_normal(n)
    mg = make_mgmc(name, 1.1, O.SOR_SYMMETRIC, "cholsampler")
    yd = dev(np.zeros(n))
    mg.sample(dev(b), yd, 2, seed=7, counter0=0, guesszero=True)
    want = oracle_mgmc(name, b, np.zeros(n), 2, 7, 0, True, 1.1, O.SOR_SYMMETRIC, "cholsampler")[-1]
    assert rel(host(yd), want) < TOL
    mg.destroy()


@pytest.mark.parametrize("nchains", [3, 65])
def test_mgmc_chains_are_the_single_chains(nchains):
    import torch

    name = "sa3d25"
    n = hier(name)[0][-1][0].shape[0] - 1
    rng = np.random.default_rng(33)
    b, Y0 = dev(rng.standard_normal(n)), dev(rng.standard_normal((n, nchains)))
    mg = make_mgmc(name, 1.1, O.SOR_SYMMETRIC, "cholsampler")
    Y = Y0.clone()
    ctr = mg.sample_chains(b, Y, 3, SEEDS[:nchains], counter0=1)
    for c in range(nchains):
        y = Y0[:, c].contiguous()
        assert mg.sample(b, y, 3, SEEDS[c], counter0=1) == ctr
        assert torch.equal(Y[:, c], y), c
    mg.destroy()


def test_mgmc_idx64_is_the_idx32_chain():
    name = "salshape"
    n = hier(name)[0][-1][0].shape[0] - 1
    rng = np.random.default_rng(34)
    b, y0 = rng.standard_normal(n), rng.standard_normal(n)
    out = []
    for w in (32, 64):
        mg = make_mgmc(name, 1.1, O.SOR_SYMMETRIC, "gibbs", idx_width=w)
        yd = dev(y0)
        mg.sample(dev(b), yd, 3, seed=5, counter0=0)
        out.append(host(yd))
        mg.destroy()
    assert np.array_equal(out[0], out[1])


# --- negative controls -------------------------------------------------------------------------------------------------------
def test_control_sweep_reaches_the_last_entry_of_the_widest_row():
    """the oracle's copy loses the last stored entry of the widest operator row: the bit-exact sweep comparison must fail"""
    from parmgmc_amd import MCSOR

    A = matrix("sa3d25-L1")
    r = int(np.argmax(np.diff(A.rowptr)))
    assert np.diff(A.rowptr)[r] - 1 >= 150
    k = A.rowptr[r + 1] - 1
    assert A.colidx[k] != r and A.vals[k] != 0
    keep = np.ones(len(A.colidx), bool)
    keep[k] = False
    rp = A.rowptr.copy()
    rp[r + 1:] -= 1
    B = O.CSR(rp, A.colidx[keep], A.vals[keep])
    cols = oracle_colors("sa3d25-L1", "greedy")
    rng = np.random.default_rng(35)
    b, y0 = rng.standard_normal(A.n), rng.standard_normal(A.n)
    mc = MCSOR(A.rowptr, A.colidx, A.vals).setup()
    yd = dev(y0)
    mc.apply(dev(b), yd)
    got = host(yd)
    assert np.array_equal(got, O.mcsor_apply(A, cols, b, y0))
    bad = O.mcsor_apply(B, cols, b, y0)
    assert not np.array_equal(got, bad) and got[r] != bad[r]
    mc.destroy()


def test_control_chain_reads_the_tail_of_the_longest_pt_row():
    """The oracle's copy of P loses one entry far down the longest P^T row (2 980 entries): the last one whose contribution
    the chain can see, i.e. the last with |v| >= 1e-2 x the row's largest entry (position 2 939).  The sampler must match
    the unchanged oracle at 1e-11 and miss the changed one by more than 100 x that, so it reads this entry.  Jacobi smoothing
    leaves the entries behind it nearly cancelled (the very last is about 1e-20), and no single entry, scaled by 1 + 1e-6,
    moves the chain past the tolerance: the largest moves it by 5e-12."""
    name = "sa3d25"
    ops, ps = hier(name)
    l = max(range(1, len(ps)), key=lambda q: np.bincount(ps[q][1]).max())
    nf, nc = len(ops[l][0]) - 1, len(ops[l - 1][0]) - 1
    P = W.as_scipy(ps[l], (nf, nc)).copy()
    j = int(np.argmax(np.bincount(P.indices, minlength=nc)))
    row = np.flatnonzero(P.indices == j)  # P^T row j, in storage order: P's rows ascending
    assert len(row) >= 1000
    v = np.abs(P.data[row])
    pos = int(np.flatnonzero(v >= 1e-2 * v.max())[-1])
    assert pos >= 1000 and pos >= 0.95 * len(row), (pos, len(row))  # far past a cap of 256 (or 1 000) entries per row
    P.data[row[pos]] = 0.0
    n = ops[-1][0].shape[0] - 1
    rng = np.random.default_rng(36)
    b, y0 = rng.standard_normal(n), rng.standard_normal(n)
    mg = make_mgmc(name, 1.1, O.SOR_SYMMETRIC, "cholsampler")
    yd = dev(y0)
    mg.sample(dev(b), yd, 3, seed=0xD00D, counter0=1)
    got = host(yd)
    assert rel(got, oracle_mgmc(name, b, y0, 3, 0xD00D, 1, False, 1.1, O.SOR_SYMMETRIC, "cholsampler")[-1]) < TOL
    assert rel(got, oracle_mgmc(name, b, y0, 3, 0xD00D, 1, False, 1.1, O.SOR_SYMMETRIC, "cholsampler", P_override={l: P})[-1]) > 100 * TOL
    mg.destroy()
