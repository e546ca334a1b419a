"""The two coloured block Gibbs kernels on colour launches of many tiles (tests/blockgibbs_geometry_cases.py: 1 to 65 tiles per
launch where tests/test_gpu_blockgibbs.py has at most 3): wavefront 3 of a workgroup, workgroups beyond the first, the early
exit next to working wavefronts, the XCD band mapping of the chains kernel at band 2 to 9 with partly and wholly idle XCDs,
tile0 and the tile offsets of up to 161 tiles, slot numbers up to 7 830, widths that change inside a launch.

  a  apply, sweep_xi         bit-equal to the cached walk-through with the library's own W under the three sweep types; rows in no
                             block and layout padding unchanged; the byte model holds the library's tile widths to the restated plan
  b  sample                  a twin handle on the same blocks coloured with at most 2 tiles per colour (the geometry the small
                             cases tie to the oracle's normals) gives the same bits and counter: the slot stream is keyed by slot,
                             not by tile, and gapped blocks are independent.  One forward sample of gap-g8 against sweep_xi fed
                             the oracle's normals, block by block by NORMAL_TOL (Walk.independent_noise_bound)
  c  chains kernel           every column of apply_chains, sample_chains (shared b, one b per chain) and sweep_xi_chains equals
                             the single-chain call, C in 1, 8, 9, 16, 17; Y 8 bytes off a 16-byte boundary between sentinels
  d  get_block_factor        every block of gap-g64 and ex6-33-stars against inv(cholesky(A_PP)) by fwd_bound(m, kappa)
  e  pos * C beyond 2^31     rows in the last 118 positions of a layout of 2^31 / 34 + 200 positions, 34 chains, against a twin
                             handle with the positions compacted

Every comparison is bit for bit (the int64 view) except the bounds of b (NORMAL_TOL of tests/woodbury_cases.py) and d
(fwd_bound of tests/chol_edge_refs.py).

Checked once against two scratch builds of the library that only skip work (neither can read or write out of bounds):
  1. the single-chain kernel returns at once for wv == 3 or blockIdx.x >= 1: a fails on all seven cases, on the gapped cases in
     exactly the colours of 4 and more tiles from tile 3 on (133 of the 161 tiles of gap-g*, 22 of the 31 of gap-mixed) and in
     no tile of the 1-tile and 3-tile colours; b and c fail with it (25 of the 30 tests; d and e pass);
  2. the chains kernel maps tiles as if band were 1 (tl = xcd): c fails on all seven cases, on the gapped cases in exactly the
     colours of 9 and more tiles from tile 8 on (100 tiles of gap-g*, 10 of gap-mixed) and in no tile of the colours of at most
     8; both sentinel tests fail; a, b, d and e, which do not call the chains kernel on more than 8 tiles, pass (21 of 30).
On wide-band and ex6-33-stars the blocks are coupled, so a skipped tile also changes tiles that are swept after it.
"""
from collections import namedtuple

import numpy as np
import pytest

import blockgibbs_geometry_cases as K
import oracle as O
import test_gpu_blockgibbs as BG
import test_gpu_blockgibbs_chains as CH
from blockgibbs_cases import BWD, FWD, SYM, colors_valid, directions, first_fit_colors, slot_offsets, star_blocks
from chol_edge_refs import fwd_bound
from woodbury_cases import NORMAL_TOL

pytestmark = pytest.mark.gpu
TYPES = (FWD, BWD, SYM)
GOLDEN = CH.GOLDEN
COUNTER0 = 2**32 + 5
dev, host, bits = BG.dev, BG.host, CH.bits

Geo = namedtuple("Geo", "c col ld pos bg Ws walk plan")
_made, _twins = {}, {}


def geo(name) -> Geo:
    """the case, its colouring, layout, handle, the library's W per block, the cached walk-through and the restated plan, built once"""
    if name not in _made:
        c = K.case(name)
        bg = BG.make(c.A, c.blocks, c.colors, c.layout)
        col = bg.get_coloring()
        assert np.array_equal(col, first_fit_colors(c.A, c.blocks) if c.colors is None else c.colors)
        assert colors_valid(c.A, c.blocks, col) and bg.get_num_colors() == col.max() + 1 and bg.get_num_slots() == sum(len(p) for p in c.blocks)
        plan = K.predicted_plan(c.blocks, col)
        assert K.tiles_per_color(plan) == K.TILES[name]
        ld, pos = K.layout_of(c)
        Ws = [bg.block_factor(p) for p in range(len(c.blocks))]
        _made[name] = Geo(c, col, ld, pos, bg, Ws, K.Walk(c.A, c.blocks, Ws, pos), plan)
    return _made[name]


def twin(name):
    """a second handle on the blocks of a gap case, coloured with at most 2 tiles per colour"""
    if name not in _twins:
        c = K.case(name)
        tw = BG.make(c.A, c.blocks, c.twin)
        assert np.array_equal(tw.get_coloring(), c.twin) and max(K.tiles_per_color(K.predicted_plan(c.blocks, c.twin))) <= 2
        _twins[name] = tw
    return _twins[name]


def vectors(ld, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(ld), rng.standard_normal(ld)


# ---- a. the single-chain kernel against the walk-through ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.NAMES)
def test_apply_and_sweep_xi_equal_the_walk_through_bit_for_bit(name):
    g = geo(name)
    bg, ns = g.bg, g.bg.get_num_slots()
    # the factor bytes of the library's plan are those of the restated one: the launches below have the tiles the case claims
    assert bg.algorithmic_bytes() == K.predicted_bytes(g.plan, g.walk.nnz_ext(), ns)
    b, y = vectors(g.ld, 1)
    xi = [np.random.default_rng(2 + d).standard_normal(ns) for d in range(2)]
    bd = dev(b)
    untouched = K.untouched_positions(g.c)
    try:
        for t in TYPES:
            bg.set_sweep_type(t)
            yd = dev(y)
            bg.apply(bd, yd)
            got, want = host(yd), g.walk.apply(g.col, b, y, t)
            assert K.same_bits(got, want), (name, t, "apply", _where(g, got, want))
            assert K.same_bits(got[untouched], y[untouched])
            yd = dev(y)
            for d, dr in enumerate(directions(t)):
                bg.sweep_xi(dev(xi[d]), bd, yd, backward=dr == BWD)
            got, want = host(yd), g.walk.apply(g.col, b, y, t, lambda d: xi[d])
            assert K.same_bits(got, want), (name, t, "sweep_xi", _where(g, got, want))
            assert K.same_bits(got[untouched], y[untouched])
    finally:
        bg.set_sweep_type(FWD)
    # negative control: one wrong bit in the last row of a block of the last tile
    p_last = int(np.argmax(g.plan.tile[slot_offsets(g.c.blocks)[:-1]]))
    want[g.pos[g.c.blocks[p_last][-1]]] *= 1 + 2.0**-52
    assert not K.same_bits(got, want)


def _where(g: Geo, got, want):
    """(colour, tile of the colour) of the slots that differ, for the failure message"""
    off = slot_offsets(g.c.blocks)
    out = set()
    for p, P in enumerate(g.c.blocks):
        if not K.same_bits(got[g.pos[P]], want[g.pos[P]]):
            out.add((int(g.col[p]), int(g.plan.tile[off[p]] - g.plan.ctile[g.col[p]])))
    return f"{len(out)} tiles differ, colours {sorted({c for c, _ in out})}, first {sorted(out)[:6]}"


# ---- b. drawn normals at many tiles ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweep", [FWD, SYM], ids=["forward", "symmetric"])
@pytest.mark.parametrize("name", K.GAP_NAMES)
def test_sample_equals_a_twin_of_at_most_two_tiles_per_colour(name, sweep):
    import torch

    g, tw = geo(name), twin(name)
    b, y = vectors(g.ld, 6)
    bd, seed = dev(b), (GOLDEN + 17) & (2**64 - 1)
    try:
        g.bg.set_sweep_type(sweep), tw.set_sweep_type(sweep)
        ya, yb = dev(y), dev(y)
        ca, cb = g.bg.sample(bd, ya, 2, seed=seed, counter0=COUNTER0), tw.sample(bd, yb, 2, seed=seed, counter0=COUNTER0)
        assert ca == cb == COUNTER0 + 2 * len(directions(sweep))
        assert torch.equal(bits(ya), bits(yb)), (name, sweep, _where(g, host(ya), host(yb)))
        assert bool(torch.isfinite(ya).all()) and not torch.equal(ya, dev(y))
        # negative controls: the next counter and another seed are other chains in every block
        rows = torch.as_tensor(np.concatenate(g.c.blocks), device="cuda")
        for kw in (dict(seed=seed, counter0=COUNTER0 + 1), dict(seed=seed ^ (1 << 63), counter0=COUNTER0)):
            yc = dev(y)
            tw.sample(bd, yc, 2, **kw)
            assert bool((yc[rows] != ya[rows]).all())
    finally:
        g.bg.set_sweep_type(FWD), tw.set_sweep_type(FWD)


def test_sample_against_injected_oracle_normals_block_by_block():
    g = geo("gap-g8")
    bg, ns = g.bg, g.bg.get_num_slots()
    b, y = vectors(g.ld, 7)
    bd, seed = dev(b), 0xCAFE
    bg.set_sweep_type(FWD)
    yd = dev(y)
    assert bg.sample(bd, yd, 1, seed=seed, counter0=COUNTER0) == COUNTER0 + 1
    got = host(yd)

    def fed(counter):
        xi = O.noise_rows(ns, seed, counter)
        yf = dev(y)
        bg.sweep_xi(dev(xi), bd, yf)
        return host(yf), float(np.abs(xi).max())

    want, xs = fed(COUNTER0)
    e = g.walk.independent_noise_bound(g.ld, NORMAL_TOL, max(float(np.abs(y).max()), float(np.abs(want).max())), float(np.abs(b).max()), xs)
    rows = np.concatenate(g.c.blocks)
    diff = np.abs(got - want)
    ratio = K.worst_ratio(diff[rows], e[rows])
    print(f"gap-g8, {ns} slots, tiles per colour {K.TILES['gap-g8']}: max |sample - fed| = {diff.max():.3g}, max ratio to the bound {ratio:.3g}")
    assert np.all(diff <= e) and (e[rows] > 0).all()
    shifted = np.abs(got - fed(COUNTER0 + 1)[0])  # negative control: the counter shifted by one is another chain
    assert shifted.max() > 1e6 * e.max() and np.median(shifted[rows]) > 1e6 * e.max()


# ---- c. the chains kernel against the single-chain kernel --------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.NAMES)
def test_every_column_equals_the_single_chain_call(name):
    import torch

    g = geo(name)
    bg, ld, ns = g.bg, g.ld, g.bg.get_num_slots()
    seen = set()
    try:
        for k, C in enumerate(K.CHAINS):
            t = TYPES[(K.NAMES.index(name) + k) % 3]
            seen.add(t)
            bg.set_sweep_type(t)
            b, B, Y0, Xi = CH._inputs(ld, ns, C, 200 + C)
            seeds = [(GOLDEN + 3 * c) & (2**64 - 1) for c in range(C)]

            def check(Y, want, what):
                if not torch.equal(bits(Y), bits(want)):
                    bad = [c for c in range(C) if not torch.equal(bits(Y[:, c]), bits(want[:, c]))]
                    raise AssertionError((name, C, t, what, f"columns {bad}", _where(g, host(Y[:, bad[0]]), host(want[:, bad[0]]))))

            Y = Y0.clone()
            bg.apply_chains(b, Y)
            want, _ = CH._columns(C, lambda c, y: bg.apply(b, y), Y0)
            check(Y, want, "apply")
            assert not torch.equal(Y, Y0)
            Y = Y0.clone()
            ctr = bg.sample_chains(b, Y, 2, seeds, counter0=COUNTER0)
            want, ctrs = CH._columns(C, lambda c, y: bg.sample(b, y, 2, seed=seeds[c], counter0=COUNTER0), Y0)
            check(Y, want, "sample")
            assert set(ctrs) == {ctr} and ctr == COUNTER0 + 2 * len(directions(t))
            Y = Y0.clone()
            ctr = bg.sample_chains(B, Y, 2, seeds, counter0=COUNTER0)
            want, ctrs = CH._columns(C, lambda c, y: bg.sample(B[:, c].contiguous(), y, 2, seed=seeds[c], counter0=COUNTER0), Y0)
            check(Y, want, "sample_rhs")
            assert set(ctrs) == {ctr}
            for backward in (False, True):
                Y = Y0.clone()
                bg.sweep_xi_chains(Xi, b, Y, backward=backward)
                want, _ = CH._columns(C, lambda c, y: bg.sweep_xi(Xi[:, c].contiguous(), b, y, backward=backward), Y0)
                check(Y, want, ("sweep_xi", backward))
    finally:
        bg.set_sweep_type(FWD)
    assert seen == set(TYPES)


@pytest.mark.parametrize("name,C", [("gap-mixed", 10), ("ex6-33-stars", 16)])
def test_nothing_else_is_written_off_a_16_byte_boundary(name, C):
    """Y one double behind a 16-byte boundary inside a larger buffer, C even: the 8-byte instance of the chains kernel for the
    alignment alone, in launches of 17 (gap-mixed) and 16 to 19 (ex6-33-stars) tiles, band 2 and 3.  Sentinels in front and behind,
    a second pattern on the rows in no block (gap-mixed) and the unused layout positions (ex6-33-stars)."""
    import torch

    g = geo(name)
    bg, ld, ns = g.bg, g.ld, g.bg.get_num_slots()
    assert max(K.TILES[name]) >= 17
    rng = np.random.default_rng(7)
    lead, tail = 5, 64
    buf = torch.full((lead + ld * C + tail,), -1.5e300, dtype=torch.float64, device="cuda")
    Y = buf[lead : lead + ld * C].view(ld, C)
    assert buf.data_ptr() % 16 == 0 and Y.is_contiguous() and Y.data_ptr() % 16 == 8 and C % 2 == 0
    Y0 = dev(rng.standard_normal((ld, C)))
    rest = torch.as_tensor(K.untouched_positions(g.c), device="cuda")
    assert len(rest) > 0
    Y0[rest] = dev(3.0e5 + np.arange(len(rest) * C).reshape(len(rest), C))
    b, B, Xi = dev(rng.standard_normal(ld)), dev(rng.standard_normal((ld, C))), dev(rng.standard_normal((ns, C)))
    seeds = list(range(40, 40 + C))
    live = torch.as_tensor(np.setdiff1d(np.arange(ld), K.untouched_positions(g.c)), device="cuda")
    try:
        for t in TYPES:
            bg.set_sweep_type(t)
            for call in (lambda Z: bg.apply_chains(b, Z), lambda Z: bg.sample_chains(b, Z, 2, seeds), lambda Z: bg.sample_chains(B, Z, 1, seeds), lambda Z: bg.sweep_xi_chains(Xi, b, Z, backward=t == BWD)):
                Y.copy_(Y0)
                before = buf.clone()
                call(Y)
                Z = Y0.clone()  # the same call on a 16-byte aligned copy: the other instance of the kernel
                assert Z.data_ptr() % 16 == 0
                call(Z)
                torch.cuda.synchronize()
                assert torch.equal(bits(buf[:lead]), bits(before[:lead])) and torch.equal(bits(buf[lead + ld * C :]), bits(before[lead + ld * C :]))
                assert torch.equal(bits(Y[rest]), bits(Y0[rest]))
                assert torch.equal(bits(Y), bits(Z)) and bool((Y[live] != Y0[live]).all()) and bool(torch.isfinite(Y).all())
    finally:
        bg.set_sweep_type(FWD)


# ---- d. block factors at scale -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gap-g64", "ex6-33-stars"])
def test_block_factors(name):
    g = geo(name)
    refs, kappas = K.numpy_factors(g.c.A, g.c.blocks)
    worst = 0.0
    for p, (W, R, kappa) in enumerate(zip(g.Ws, refs, kappas)):
        assert W.shape == R.shape and np.array_equal(W, np.tril(W))
        err, bound = np.abs(W - R).max(), fwd_bound(len(g.c.blocks[p]), kappa) * np.abs(R).max()
        worst = max(worst, err / bound)
        assert err <= bound, (name, p, err, bound)
    print(f"{name}, {len(refs)} blocks: max |W - inv(chol(A_PP))| / bound = {worst:.3g}")
    # negative control: the bound sees a relative change of 1e-9 in the last diagonal entry of the last block
    bad = g.Ws[-1].copy()
    bad[-1, -1] *= 1 + 1e-9
    assert np.abs(bad - refs[-1]).max() > fwd_bound(len(g.c.blocks[-1]), kappas[-1]) * np.abs(refs[-1]).max()


# ---- e. row offsets beyond 2^31 elements -------------------------------------------------------------------------------------------
def test_rows_whose_offset_passes_2_to_the_31():
    """the `layout` operator and stars of tests/test_gpu_blockgibbs.py in a layout of 2^31 / 34 + 200 positions, 34 chains: 41 rows
    sit in the last 118 positions, where pos * C does not fit 32 bits; the other 40 below position 200.  Y is allocated, never
    filled: only the 81 positions and sentinel rows around them are written.  A twin handle has the positions compacted."""
    import torch

    C, n = 34, 81
    ld = 2**31 // C + 200
    need = 24 * 2**30
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{free / 2**30:.1f} GiB of device memory free, the test wants 24 GiB")
    A = O.ex6_matrix(9, 0.05)
    blocks = star_blocks(A)
    rng = np.random.default_rng(31)
    low, high = rng.permutation(200)[:40], ld - 118 + rng.permutation(118)[:41]
    pos = rng.permutation(np.concatenate([low, high]))
    assert len(pos) == n and (high.astype(np.int64) * C > 2**31).all() and (low < 200).all() and ld * C * 8 > 17.1e9
    order = np.argsort(np.argsort(pos))  # the same positions in the same order, compacted
    pos2, ld2 = 7 + order, n + 37
    big, small = BG.make(A, blocks, None, (ld, pos)), BG.make(A, blocks, None, (ld2, pos2))
    ns = big.get_num_slots()
    assert np.array_equal(big.get_coloring(), small.get_coloring())
    guard = 8  # sentinel rows below the high positions; above them the buffer goes on for `tail` doubles
    tail = 64
    lo_rows = torch.arange(0, 200 + guard, device="cuda")
    hi_rows = torch.arange(ld - 118 - guard, ld, device="cuda")
    tpos, tpos2 = torch.as_tensor(pos, device="cuda"), torch.as_tensor(pos2, device="cuda")
    buf = torch.empty(ld * C + tail, dtype=torch.float64, device="cuda")
    Y = buf[: ld * C].view(ld, C)
    b = torch.empty(ld, dtype=torch.float64, device="cuda")
    bv, Y0, Xi = dev(rng.standard_normal(n)), dev(rng.standard_normal((n, C))), dev(rng.standard_normal((ns, C)))
    b[tpos] = bv
    b2 = torch.zeros(ld2, dtype=torch.float64, device="cuda")
    b2[tpos2] = bv
    seeds = [(GOLDEN + 5 * c) & (2**64 - 1) for c in range(C)]
    sent = dev(-7.0e5 - np.arange((200 + guard) * C).reshape(200 + guard, C))
    senth = dev(9.0e5 + np.arange((118 + guard) * C).reshape(118 + guard, C))
    keep_lo = torch.as_tensor(np.setdiff1d(np.arange(200 + guard), low), device="cuda")
    keep_hi = torch.as_tensor(np.setdiff1d(np.arange(118 + guard), high - (ld - 118 - guard)), device="cuda")
    try:
        for what, call in (("apply", lambda h, bb, Z: h.apply_chains(bb, Z)), ("sample", lambda h, bb, Z: h.sample_chains(bb, Z, 2, seeds, counter0=COUNTER0)), ("sweep_xi", lambda h, bb, Z: h.sweep_xi_chains(Xi, bb, Z))):
            for h in (big, small):
                h.set_sweep_type(SYM if what == "sample" else FWD)
            Y[lo_rows], Y[hi_rows] = sent, senth
            buf[ld * C :] = -1.5e300
            Y[tpos] = Y0
            Z = torch.zeros(ld2, C, dtype=torch.float64, device="cuda")
            Z[tpos2] = Y0
            ra, rb = call(big, b, Y), call(small, b2, Z)
            torch.cuda.synchronize()
            assert ra == rb
            got, want = Y[tpos], Z[tpos2]
            assert torch.equal(bits(got), bits(want)), (what, [int(r) for r in torch.nonzero((got != want).any(dim=1)).flatten()[:8]])
            assert bool((got != Y0).all()) and bool(torch.isfinite(got).all())
            assert torch.equal(bits(Y[lo_rows][keep_lo]), bits(sent[keep_lo])) and torch.equal(bits(Y[hi_rows][keep_hi]), bits(senth[keep_hi])), what
            assert bool((buf[ld * C :] == -1.5e300).all())
        # negative control: the comparison sees one wrong bit in a row beyond 2^31
        want = want.clone()
        r = int(np.argmax(pos))
        want[r, C - 1] = torch.nextafter(want[r, C - 1], want[r, C - 1] + 1)
        assert not torch.equal(bits(got), bits(want))
    finally:
        del buf, Y, b
        big.destroy(), small.destroy()
        torch.cuda.empty_cache()
