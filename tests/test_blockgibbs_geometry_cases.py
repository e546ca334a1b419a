"""tests/blockgibbs_geometry_cases.py without a GPU: the restated constants and launch arithmetic are the sources', every case
has a valid colouring and the tiles per colour it is there for, the restated launch maps serve every (tile, chunk) of every
launch once with the idle workgroups counted, the sparse band operator is blockgibbs_cases.banded, the cached walk-through has
the bits of walk_sweep, a sweep over the gapped blocks does not depend on the colouring, and the negative controls are seen."""
import re
from pathlib import Path

import numpy as np
import pytest

import blockgibbs_geometry_cases as K
import oracle as O
from blockgibbs_cases import BWD, FWD, SYM, banded, colors_valid, consecutive_blocks, first_fit_colors, star_blocks, walk_apply, walk_sweep

CSRC = Path(__file__).resolve().parent.parent / "parmgmc_amd" / "csrc"


def _src(name):
    return re.sub(r"\s+", " ", (CSRC / name).read_text())


def colors_of(c):
    return first_fit_colors(c.A, c.blocks) if c.colors is None else c.colors


def test_restated_constants_are_the_sources():
    single, chains, host = _src("kernels_blockgibbs.hip"), _src("kernels_blockgibbs_chains.hip"), _src("pmg_blockgibbs_host.c")
    assert "__launch_bounds__(256) void blockgibbs_color_kernel" in single and "const dim3 block(256), grid((ntiles + 3) / 4);" in single
    assert "const int tl = blockIdx.x * (blockDim.x >> 6) + wv; if (tl >= ntiles) return;" in single
    assert "lane = threadIdx.x & 63, wv = threadIdx.x >> 6;" in single and "__shared__ double s_line[4][2][64];" in single
    assert "constexpr int CB = 8;" in chains and K.CB == 8 and "__launch_bounds__(64) void blockgibbs_color_chains_kernel" in chains
    assert "const int band = (ntiles + 7) / 8;" in chains and "const int nchunks = (C + CB - 1) / CB;" in chains
    assert "std::min<int64_t>(nchunks, std::max<int64_t>(1, ((int64_t)1 << 30) / (8 * (int64_t)band)));" in chains and K.MAX_GRID == 1 << 30
    assert "const dim3 block(64), grid(8u * (unsigned)band * (unsigned)ny);" in chains
    assert "const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3; const int tl = xcd * band + k / ny; if (tl >= ntiles) return;" in chains
    assert "for (int chunk = k % ny; chunk < nchunks; chunk += ny) {" in chains
    assert "static int padded_width(int m) { return m <= 8 ? 8 : m <= 16 ? 16 : m <= 32 ? 32 : 64; }" in host
    assert "const int per = 64 / (8 << (q & 3));" in host and "first[q + 1] = first[q] + (cnt[q] + per - 1) / per;" in host
    assert [K.padded_width(m) for m in (1, 8, 9, 16, 17, 32, 33, 64)] == [8, 8, 16, 16, 32, 32, 64, 64]


@pytest.mark.parametrize("name", K.NAMES)
def test_case_has_the_tiles_it_is_there_for(name):
    c = K.case(name)
    A, blocks, col = c.A, c.blocks, colors_of(c)
    assert A.n <= 8600 and A.colidx.dtype == np.int32 and len(col) == len(blocks)
    assert colors_valid(A, blocks, col)
    plan = K.predicted_plan(blocks, col)
    assert K.tiles_per_color(plan) == K.TILES[name] and K.check_plan(plan, blocks, col) == []
    assert max(K.TILES[name]) >= 17 and plan.ctile[-1] == sum(K.TILES[name])
    rows = np.concatenate(blocks)
    if name in K.GAP_NAMES:  # one gap row between neighbours and one behind the last block: the blocks are independent
        assert len(np.unique(rows)) == len(rows) and all(blocks[p + 1][0] == blocks[p][-1] + 2 for p in range(len(blocks) - 1)) and A.n == blocks[-1][-1] + 2
        assert np.diff(A.rowptr).max() == 3 and len(K.untouched_positions(c)) == len(blocks)
        tw = K.predicted_plan(blocks, c.twin)
        assert colors_valid(A, blocks, c.twin) and max(K.tiles_per_color(tw)) <= 2 and K.check_plan(tw, blocks, c.twin) == []
    if name[:5] == "gap-g":
        g = int(name[5:])
        lo, hi = K._size_range(g)
        assert K.tiles_per_color(plan) == K.TARGET_TILES == (1, 3, 4, 5, 8, 9, 16, 17, 33, 65) and set(plan.tile_g) == {g}
        fills = [K.last_tile_blocks(plan, blocks, col, k, g) for k in range(10)]
        assert fills == [1 + k % (64 // g) for k in range(10)]  # full and partial last tiles (one block per tile at g = 64)
        for k in range(10):  # every colour holds every size of its width class where it has the blocks for it
            sizes = {len(blocks[p]) for p in np.flatnonzero(col == k)}
            assert sizes <= set(range(lo, hi + 1)) and (len(sizes) == hi - lo + 1 or (col == k).sum() < 4 * (hi - lo + 1))
        assert {len(P) for P in blocks} == set(range(lo, hi + 1))
    if name == "gap-mixed":
        for k, tiles in enumerate(K.MIXED_TILES):
            tg = plan.tile_g[plan.ctile[k] : plan.ctile[k + 1]]
            assert [int((tg == g).sum()) for g in K.WIDTHS] == list(tiles)
            for g in K.WIDTHS[:3]:  # the last tile of a width group is partial
                assert K.last_tile_blocks(plan, blocks, col, k, g) == K.mixed_last_fill(g, k) < 64 // g
        tg = plan.tile_g[plan.ctile[2] :]  # the 17-tile launch: widths change inside a workgroup of four tiles and between two
        quads = [set(tg[i : i + 4].tolist()) for i in range(0, 17, 4)]
        assert any(len(q) > 1 for q in quads) and len({tuple(sorted(q)) for q in quads}) > 2
    if name == "wide-band":
        assert A.n == 3191 and len(blocks) == 532 and np.diff(A.rowptr).max() == 23 and len(np.unique(rows)) == A.n
        for k in range(4):  # same-colour blocks are at least 13 rows apart: more than the half-bandwidth
            mine = [blocks[p] for p in np.flatnonzero(col == k)]
            assert min(mine[i + 1][0] - mine[i][-1] for i in range(len(mine) - 1)) >= 13 > 11
        w = K.Walk(A, blocks[:40], [np.eye(len(P)) for P in blocks[:40]])
        ew = sorted({int(el.max()) for _, _, el in w.ext[8:]})  # blocks with the whole band on both sides
        assert ew[0] >= 15 and ew[-1] == 19 and any(e % 4 for e in ew)  # past the batch edges 8 and 16, an end inside a group of 4
    if name == "ex6-33-stars":
        ld, pos = K.layout_of(c)
        assert len(blocks) == 1089 and ld == 1089 + 37 and len(np.unique(pos)) == 1089 and len(rows) > len(np.unique(rows)) == A.n
        assert len(K.untouched_positions(c)) == 37


def _tile_counts():
    out = set()
    for name in K.NAMES:
        c = K.case(name)
        out |= set(K.TILES[name])
        if c.twin is not None:
            out |= set(K.tiles_per_color(K.predicted_plan(c.blocks, c.twin)))
    return sorted(out)


def test_launch_maps_serve_every_tile_and_chunk_once():
    counts = _tile_counts()
    assert set(K.TARGET_TILES) | {2, 18, 19} <= set(counts)
    for nt in counts:
        served, idle = K.single_served(nt)
        grid = K.single_grid(nt)
        assert grid == -(-nt // 4) and sorted(tl for _, _, tl in served) == list(range(nt)) and idle == 4 * grid - nt
        assert all(K.single_home(tl) == (wg, wv) for wg, wv, tl in served)
        assert (3 in {wv for _, wv, _ in served}) == (nt >= 4) and (max(wg for wg, _, _ in served) >= 1) == (nt >= 5)
        for C in K.MAP_CHAINS:
            L = K.chains_launch(nt, C)
            assert L.band == -(-nt // 8) and L.nchunks == L.ny == -(-C // 8) and L.grid == 8 * L.band * L.ny
            assert K.chains_cover(L), (nt, C)
            assert all(len(K.chains_served(L, w)) <= 1 for w in range(L.grid))  # the chunk loop runs once
            assert K.idle_workgroups(L) == (8 * L.band - nt) * L.ny
            assert K.idle_xcds(L) == 8 - -(-nt // L.band)
    # the figures of the cases
    L = K.chains_launch(9, 8)
    assert (L.band, L.grid, K.idle_workgroups(L), K.idle_xcds(L)) == (2, 16, 7, 3)
    assert K.chains_served(L, 4) == [(8, 0)] and K.chains_served(L, 12) == []  # XCD 4: one tile of its band of two
    for nt, band, idle, xcds in ((1, 1, 7, 7), (8, 1, 0, 0), (16, 2, 0, 0), (17, 3, 7, 2), (33, 5, 7, 1), (65, 9, 7, 0)):
        L = K.chains_launch(nt, 17)
        assert (L.band, L.ny, K.idle_workgroups(L), K.idle_xcds(L)) == (band, 3, 3 * idle, xcds), nt
    # beyond the launch limit the chunks go into the kernel's loop and are still served once
    L = K.ChainsLaunch(nt=5, band=1, nchunks=7, ny=3, grid=8 * 3)
    assert K.chains_cover(L) and max(len(K.chains_served(L, w)) for w in range(L.grid)) == 3
    assert K.chains_launch(8 << 27, 17).ny == 1 and K.chains_launch(8 << 26, 17).ny == 2


def test_sparse_band_operator_is_the_dense_rule():
    for n, hb, seed in ((60, 1, 13), (80, 11, 5), (300, 70, 11)):
        S, D = K.banded_sparse(n, hb, seed), banded(n, hb, seed)
        assert np.array_equal(S.rowptr, D.rowptr) and np.array_equal(S.colidx, D.colidx)
        d = S.colidx == np.repeat(np.arange(n), np.diff(S.rowptr))
        assert np.array_equal(S.vals[~d], D.vals[~d])  # the same draws
        assert np.allclose(S.vals[d], D.vals[d], rtol=4 * hb * 2.0**-53, atol=0)  # the row sums in another order
        off = np.abs(S.scipy()).sum(axis=1).A1 - S.vals[d]
        assert (S.vals[d] > off + 0.99).all() and (abs(S.scipy() - S.scipy().T)).nnz == 0


def _small_case(name):
    if name == "band":  # consecutive blocks of every width class but the widest on a band of half-width 5, two rows in no block
        return K.banded_sparse(90, 5, 3), consecutive_blocks([1, 7, 8, 9, 16, 17, 3], 2), None
    A = O.ex6_matrix(9, 0.05)
    return A, star_blocks(A), np.random.default_rng(5).permutation(81 + 37)[:81]


@pytest.mark.parametrize("name", ["band", "stars-layout"])
def test_cached_walk_through_has_the_bits_of_walk_sweep(name):
    A, blocks, pos = _small_case(name)
    col = first_fit_colors(A, blocks)
    Ws, _ = K.numpy_factors(A, blocks)
    ld = A.n if pos is None else 81 + 37
    rng = np.random.default_rng(1)
    b, y = rng.standard_normal(ld), rng.standard_normal(ld)
    xi = [rng.standard_normal(sum(len(P) for P in blocks)) for _ in range(2)]
    w = K.Walk(A, blocks, Ws, pos)
    for backward in (False, True):
        for x in (None, xi[0]):
            got, want = w.sweep(col, b, y, x, backward), walk_sweep(A, blocks, col, Ws, b, y, x, backward, pos)
            assert K.same_bits(got, want) and not K.same_bits(got, y)
    for t in (FWD, BWD, SYM):
        for xf in (None, lambda d: xi[d]):
            assert K.same_bits(w.apply(col, b, y, t, xf), walk_apply(A, blocks, col, Ws, b, y, t, xf, pos))
    assert w.nnz_ext() == sum(int((~np.isin(A.colidx[A.rowptr[r] : A.rowptr[r + 1]], P)).sum()) for P in blocks for r in P)


@pytest.mark.parametrize("name", K.GAP_NAMES)
def test_a_sweep_over_gapped_blocks_does_not_depend_on_the_colouring(name):
    c = K.case(name)
    Ws, _ = K.numpy_factors(c.A, c.blocks)
    w = K.Walk(c.A, c.blocks, Ws)
    rng = np.random.default_rng(2)
    b, y, xi = rng.standard_normal(c.A.n), rng.standard_normal(c.A.n), rng.standard_normal(sum(len(P) for P in c.blocks))
    gaps = K.untouched_positions(c)
    for backward in (False, True):
        for x in (None, xi):
            many, few = w.sweep(c.colors, b, y, x, backward), w.sweep(c.twin, b, y, x, backward)
            assert K.same_bits(many, few) and K.same_bits(many[gaps], y[gaps]) and (np.delete(many, gaps) != np.delete(y, gaps)).all()
    assert not K.same_bits(w.sweep(c.colors, b, y, xi), w.sweep(c.colors, b, y, None))


def test_negative_controls():
    # a plan with two width groups swapped
    c = K.case("gap-mixed")
    good, swapped = K.predicted_plan(c.blocks, c.colors), K.predicted_plan(c.blocks, c.colors, order=(8, 32, 16, 64))
    assert K.check_plan(good, c.blocks, c.colors) == []
    assert any("do not ascend" in m for m in K.check_plan(swapped, c.blocks, c.colors))
    assert K.tiles_per_color(swapped) == K.tiles_per_color(good) and not np.array_equal(swapped.tile, good.tile)
    moved = good._replace(lane=np.where(good.tile == 3, (good.lane + 8) % 64, good.lane))  # the blocks of one tile rotated by a block
    assert K.check_plan(moved, c.blocks, c.colors) != []
    # a chains launch mapped as if band were 1 loses the ninth tile; at 8 tiles it is the library's map
    assert not K.chains_cover(K.chains_launch(9, 17, band=1)) and K.chains_cover(K.chains_launch(9, 17))
    assert K.chains_cover(K.chains_launch(8, 17, band=1))
    assert not K.covered_once([(0, 0), (0, 0), (1, 0)], 2, 1) and not K.covered_once([(0, 0)], 2, 1) and K.covered_once([(1, 0), (0, 0)], 2, 1)
    # a single-chain launch of three tiles per workgroup serves tiles twice and misses the last ones
    assert sorted(tl for _, _, tl in K.single_served(9, waves=3)[0]) != list(range(9))
    # one ulp is seen by every comparison helper
    a = np.random.default_rng(3).standard_normal(50)
    b = a.copy()
    b[17] = np.nextafter(b[17], np.inf)
    assert K.same_bits(a, a.copy()) and not K.same_bits(a, b) and not K.same_bits(np.zeros(2), -np.zeros(2)) and K.same_bits(np.array([np.nan]), np.array([np.nan]))
    assert K.worst_ratio(np.abs(a - b), np.zeros(50)) == np.inf and K.worst_ratio(np.abs(a - a), np.zeros(50)) == 0.0
    assert K.worst_ratio(np.abs(a - b), np.full(50, np.abs(a - b).max() / 2)) == 2.0
