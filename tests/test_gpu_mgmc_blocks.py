"""MGMC with block Gibbs smoothing on levels of a caller-supplied hierarchy (pmg_mgmc_set_level_blocks): the reference's
examples/ex13.py:11-22 composition, PCGAMGMC whose level smoother is PCASM multiplicative around the Cholesky sampler.

The hierarchy is a 3-level plain-aggregation hierarchy on the squared ex6 operator of a 17 x 17 grid, vertex-star blocks on the
two upper levels, the exact Cholesky sampler below.  Two samples against O.gamgmc_richardson whose `smooth` is the plain numpy
block sweep of tests/blockgibbs_cases.py drawing O.noise_rows(nslots_l, level_seed(seed, l), 64 s + d): 1e-11 relative, the
tolerance of the AIJ-hierarchy parity tests (tests/test_gpu_benchsize_oracle.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import oracle as O
from blockgibbs_cases import BWD, FWD, Reference, directions, first_fit_colors, ref_sweep, squared, star_blocks

pytestmark = pytest.mark.gpu
GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
SEED = 0xCAFE


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def level_seed(seed, l):
    return (seed + GOLD * (l + 1)) & M64


_h = {}


def hierarchy():
    """(operators, interpolations, O.CSR per level, blocks per level (None on level 0))"""
    if not _h:
        from parmgmc_amd.unstructured import build_hierarchy

        e = O.ex6_matrix(17, 0.5)
        ops, ps = build_hierarchy(squared(e).scipy(), coarse_max=1, max_levels=3)
        sizes = [len(o[0]) - 1 for o in ops]
        assert len(ops) == 3 and sizes[2] == 289 and sizes[0] > 1, sizes
        csr = [O.CSR(*o) for o in ops]
        blocks = [None, star_blocks(csr[1]), star_blocks(e)]  # level 1: the stars of its own pattern; the fine level: 5-point stars
        assert max(len(p) for p in blocks[1]) <= 64
        _h["v"] = (ops, ps, csr, blocks)
    return _h["v"]


def build(nu=1, sweep=FWD, with_blocks=True):
    from parmgmc_amd import MGMC

    ops, ps, csr, blocks = hierarchy()
    mg = MGMC.from_hierarchy(ops, ps)
    mg.set_smoother(True, 1.0, sweep, nu)
    if with_blocks:
        for l in (1, 2):
            mg.set_level_blocks(l, blocks[l])
    return mg.setup()


@pytest.mark.parametrize("guesszero,nu,sweep", [(False, 1, FWD), (True, 1, FWD), (False, 2, FWD), (True, 2, O.SOR_SYMMETRIC)])
def test_two_samples_against_the_oracle_cycle(guesszero, nu, sweep):
    ops, ps, csr, blocks = hierarchy()
    sizes = [c.n for c in csr]
    mg = build(nu, sweep)
    rng = np.random.default_rng(21)
    b, y0 = rng.standard_normal(sizes[2]), rng.standard_normal(sizes[2])
    yd = dev(y0)
    assert mg.sample(dev(b), yd, 2, seed=SEED, counter0=0, guesszero=guesszero) == 2
    mats = [c.scipy() for c in csr]
    Ps = [None] + [sp.csr_matrix((p[2], p[1], p[0]), shape=(sizes[l], sizes[l - 1])) for l, p in enumerate(ps) if p is not None]
    lv = [dict(A=mats[l], P=Ps[l]) for l in range(3)]
    refs = [None] + [Reference(csr[l], blocks[l]) for l in (1, 2)]
    cols = [None] + [first_fit_colors(csr[l], blocks[l]) for l in (1, 2)]
    Lc = O.potrf_lower(csr[0].dense())
    y = y0.copy()
    for s in range(2):
        ctr = {l: 64 * s for l in range(3)}

        def draw(l, n):
            c = ctr[l]
            ctr[l] += 1
            return O.noise_rows(n, level_seed(SEED, l), c)

        def smooth(l, rhs, x, leg):
            for _ in range(nu):
                for dr in directions(sweep):
                    x = ref_sweep(refs[l], cols[l], rhs, x, draw(l, int(refs[l].off[-1])), dr == BWD)
            return x

        y = O.gamgmc_richardson(lv, b, y, 1, guesszero and s == 0, smooth, lambda rhs: O.chol_sample(Lc, rhs, draw(0, sizes[0])))
    err = np.abs(host(yd) - y).max() / np.abs(y).max()
    print(f"guesszero {guesszero} nu {nu} sweep {sweep}: relative error {err:.2e}")
    assert err < 1e-11
    # the level byte model charges the block sweeps: (factors as stored + 12 nnz_ext + 28 nslots) per directional sweep
    from parmgmc_amd import BlockGibbs

    tot, per = mg.algorithmic_bytes()
    plain_tot, plain_per = build(nu, sweep, with_blocks=False).algorithmic_bytes()
    for l in (1, 2):
        bgb = BlockGibbs(*ops[l], blocks[l]).setup().algorithmic_bytes()
        point = 12.0 * len(ops[l][1]) + 40.0 * sizes[l]
        assert per[l] - plain_per[l] == 2 * nu * len(directions(sweep)) * (bgb - point)
    assert per[0] == plain_per[0] and tot == per.sum()


def test_level_sweep_is_the_block_sweep_bit_for_bit():
    """level_sweep on a block level = BlockGibbs on the same operator in the level's layout (that of a pmg_mcsor of the operator)"""
    from parmgmc_amd import MCSOR, BlockGibbs, PMGError

    ops, ps, csr, blocks = hierarchy()
    mg = build()
    for l in (1, 2):
        mc = MCSOR(*ops[l]).setup()
        ld, pos = mc.layout_len(), mc.get_layout()
        assert mg.level_layout(l)[:2] == (2, ld)
        bg = BlockGibbs(*ops[l], blocks[l], layout=(ld, pos)).setup()
        rng = np.random.default_rng(30 + l)
        b, x = rng.standard_normal(ld), rng.standard_normal(ld)
        for backward in (False, True):
            xm, xb = dev(x), dev(x)
            mg.level_sweep(l, dev(b), xm, backward=backward)
            bg.set_sweep_type(BWD if backward else FWD)
            bg.apply(dev(b), xb)
            assert np.array_equal(host(xm), host(xb))
            xm, xb = dev(x), dev(x)
            mg.level_sweep(l, dev(b), xm, backward=backward, noisy=True, seed=level_seed(SEED, l), counter=7)
            assert bg.sample(dev(b), xb, 1, seed=level_seed(SEED, l), counter0=7) == 8
            assert np.array_equal(host(xm), host(xb)) and not np.array_equal(host(xm), x)
    with pytest.raises(PMGError) as e:  # a level without blocks keeps its answer
        build(with_blocks=False).level_sweep(2, dev(b), dev(x))
    assert e.value.code == 56


def test_without_the_setter_the_chain_is_the_point_chain():
    """a hierarchy on which set_level_blocks was never called: byte-identical to MGMC.from_hierarchy alone, before and after block
    handles lived in the process, and different from the block chain"""
    ops, ps, csr, blocks = hierarchy()
    rng = np.random.default_rng(22)
    b, y0 = rng.standard_normal(289), rng.standard_normal(289)

    def run(mg):
        yd = dev(y0)
        mg.sample(dev(b), yd, 3, seed=SEED, counter0=4)
        return host(yd)

    before = run(build(with_blocks=False))
    block = run(build())
    after = run(build(with_blocks=False))
    assert np.array_equal(before, after) and not np.array_equal(before, block)
    # ... and it is the oracle's point-Gibbs cycle, as for every AIJ hierarchy
    sizes = [c.n for c in csr]
    lv = [dict(A=csr[l].scipy(), P=None if l == 0 else sp.csr_matrix((ps[l][2], ps[l][1], ps[l][0]), shape=(sizes[l], sizes[l - 1]))) for l in range(3)]
    cols = [O.coloring_greedy(c) for c in csr]
    Lc = O.potrf_lower(csr[0].dense())
    y = y0.copy()
    for s in range(4, 7):
        ctr = {l: 64 * s for l in range(3)}

        def noise(l):
            c = ctr[l]
            ctr[l] += 1
            return O.noise_rows(sizes[l], level_seed(SEED, l), c)

        smooth = lambda l, rhs, x, leg: O.gibbs_samples(csr[l], cols[l], rhs, x, 1, lambda d: noise(l), 1.0, O.SOR_FORWARD, True)
        y = O.gamgmc_richardson(lv, b, y, 1, False, smooth, lambda rhs: O.chol_sample(Lc, rhs, noise(0)))
    assert np.abs(before - y).max() / np.abs(y).max() < 1e-11


def test_refusals():
    """what a hierarchy with a block level does not carry returns PMG_ERR_SUP (56), whichever call comes second"""
    import torch

    from parmgmc_amd import MGMC, PMGError
    from parmgmc_amd.capi import lib

    ops, ps, csr, blocks = hierarchy()

    def fresh(with_blocks):
        mg = MGMC.from_hierarchy(ops, ps)
        if with_blocks:
            mg.set_level_blocks(2, blocks[2])
        return mg

    def refused(fn):
        with pytest.raises(PMGError) as e:
            fn()
        assert e.value.code == 56, e.value
        return str(e.value)

    # omega != 1
    assert "omega" in refused(lambda: fresh(True).set_smoother(True, 1.2))
    mg = fresh(False)
    mg.set_smoother(True, 1.2)
    assert "omega" in refused(lambda: mg.set_level_blocks(2, blocks[2]))
    # a low-rank update
    B, S = np.ones((289, 2)), np.ones(2)
    assert "low-rank" in refused(lambda: fresh(True).set_lowrank(B, S))
    mg = fresh(False)
    mg.set_lowrank(B, S)
    assert "low-rank" in refused(lambda: mg.set_level_blocks(2, blocks[2]))
    # many chains per launch, before and after set-up
    Y = torch.zeros(289, 2, dtype=torch.float64, device="cuda")
    bvec = torch.zeros(289, dtype=torch.float64, device="cuda")
    assert "block" in refused(lambda: fresh(True).sample_chains(bvec, Y, 1, [1, 2]))
    assert "block" in refused(lambda: build().sample_chains(bvec, Y, 1, [1, 2]))
    assert "block" in refused(lambda: build().sample_chains(torch.zeros(289, 2, dtype=torch.float64, device="cuda"), Y, 1, [1, 2]))
    # row-block levels
    mg = fresh(True)
    i32, i64 = np.zeros(4, np.int32), np.zeros(4, np.int64)
    assert lib.pmg_mgmc_set_level_rowblock(mg._h, 2, 0, 1, 1, i32.ctypes.data, i64.ctypes.data, i32.ctypes.data, i64.ctypes.data, i64.ctypes.data, i32.ctypes.data, i32.ctypes.data) == 56
    assert lib.pmg_mgmc_set_rowblock_transport(mg._h, i64.ctypes.data, i64.ctypes.data) == 56  # refused before the transport is looked at
    # DMDA handles
    assert "DMDA" in refused(lambda: MGMC(9, 9, 1, 1.0, 2).set_level_blocks(1, blocks[1]))
    # level 0 under the exact coarse sampler is not smoothed: a wrong argument at set-up, not an unsupported one
    mg = fresh(True)
    mg.set_level_blocks(0, [np.arange(csr[0].n)])
    with pytest.raises(PMGError) as e:
        mg.setup()
    assert e.value.code == 62


def test_block_coarse_level():
    """level 0 smoothed by block sweeps when the coarse sampler is Gibbs: one block = the whole level is the exact sampler's law;
    the cycle runs and differs from the point-Gibbs coarse chain"""
    from parmgmc_amd import MGMC

    ops, ps, csr, blocks = hierarchy()
    rng = np.random.default_rng(23)
    b, y0 = rng.standard_normal(289), rng.standard_normal(289)
    out = []
    for coarse_blocks in (False, True):
        mg = MGMC.from_hierarchy(ops, ps)
        mg.set_coarse("gibbs", 2)
        for l in (1, 2):
            mg.set_level_blocks(l, blocks[l])
        if coarse_blocks:
            mg.set_level_blocks(0, [np.arange(csr[0].n)])
        mg.setup()
        yd = dev(y0)
        mg.sample(dev(b), yd, 2, seed=SEED)
        out.append(host(yd))
    assert np.isfinite(out[1]).all() and not np.array_equal(out[0], out[1])
