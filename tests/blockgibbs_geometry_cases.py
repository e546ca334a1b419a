"""Launch geometry, many-tile cases and a cached walk-through for the two coloured block Gibbs kernels (blockgibbs_color_kernel,
kernels_blockgibbs.hip; blockgibbs_color_chains_kernel, kernels_blockgibbs_chains.hip).  Importable without a device:
tests/test_blockgibbs_geometry_cases.py checks this module on the CPU, tests/test_gpu_blockgibbs_geometry.py runs the library
against it.  The cases of tests/test_gpu_blockgibbs.py launch at most 3 tiles per colour; the ones here launch 1 to 65.

  predicted_plan   the packing rule of pmg_blockgibbs_host.c restated: inside a colour the blocks of padded width 8, then 16, 32,
                   64, each group in block order, 64 / g blocks per tile; check_plan names what a plan breaks of that rule
  single_served    blockgibbs_color_kernel: 256 threads = 4 tiles per workgroup, grid = ceil(nt / 4), tile tl in workgroup tl // 4,
                   wavefront tl % 4
  chains_launch,   blockgibbs_color_chains_kernel: one tile x one chunk of CB = 8 chains per workgroup, band = ceil(nt / 8),
  chains_served    grid = 8 * band * ny, workgroup id serves tile (id % 8) * band + (id / 8) / ny and chunk (id / 8) % ny
  covered_once     every (tile, chunk) of a launch is served exactly once; idle_workgroups counts the early exits
  banded_sparse    the rule of blockgibbs_cases.banded through scipy.sparse.diags: no n x n array anywhere, n reaches 8000
  case             the cases (NAMES), built once; TILES holds the tiles per colour every case must give
  Walk             blockgibbs_cases.walk_sweep with M = gram(W) and the exterior entries of every block formed once

Which launch-geometry terms a case reaches (nt = tiles of a colour launch):
  gap-g8 .. gap-g64  nt in 1, 3, 4, 5, 8, 9, 16, 17, 33, 65 of ONE width: wavefront 3 (nt >= 4), blockIdx.x >= 1 (nt >= 5), the
                     early exit of some wavefronts of the last workgroup (nt % 4 != 0), band 1 full (8), band 2 with 7 idle
                     workgroups and 3 idle XCDs (9), band 2 full (16), band 3 (17: XCD 5 serves two tiles of three, XCDs 6 and 7
                     none), band 5 (33), band 9 (65: XCD 7 serves two tiles); tile0 up to 96, 161 tiles in all, slots up to
                     7 830; a partial last tile in every colour
  gap-mixed          the four widths in ONE launch of 5, 9 and 17 tiles: tile_g and the factor stride change inside a workgroup
                     and from one workgroup to the next
  wide-band          coupled blocks with exterior rows of 15 to 19 entries (past the IB = 8 batch edges 8 and 16, ending inside an
                     EB = 4 group) in four launches of 17 tiles
  ex6-33-stars       overlapping stars, first-fit colours of 19 .. 16 and 1 tiles, vectors in a layout with ld > n
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import oracle as O
from blockgibbs_cases import BWD, consecutive_blocks, directions, gram, slot_offsets, star_blocks, visit_order
from chol_edge_refs import gamma

WIDTHS = (8, 16, 32, 64)  # padded widths in the order a colour packs them
WAVES = 4  # tiles per workgroup of the single-chain kernel
XCDS = 8  # the chains kernel deals tile bands to 8 XCDs
CB = 8  # chains per chunk of the chains kernel
MAX_GRID = 1 << 30  # workgroups of one chains launch before chunks go into the kernel's loop

TARGET_TILES = (1, 3, 4, 5, 8, 9, 16, 17, 33, 65)  # tiles per colour of the gap-g* cases
MIXED_TILES = ((2, 1, 1, 1), (3, 2, 2, 2), (5, 4, 4, 4))  # gap-mixed: tiles of width 8, 16, 32, 64 per colour
CHAINS = (1, 8, 9, 16, 17)  # chain counts of the device tests
MAP_CHAINS = CHAINS + (65,)  # chain counts the launch maps are checked at


def padded_width(m: int) -> int:
    return 8 if m <= 8 else 16 if m <= 16 else 32 if m <= 32 else 64


def same_bits(a, b) -> bool:
    """bit for bit: unlike np.array_equal it tells -0.0 from 0.0 and takes equal NaNs as equal"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


def worst_ratio(err, bound) -> float:
    """the largest err / bound; an error where the bound is zero counts as infinite"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    safe = np.where(bound > 0, bound, 1.0)
    return float(np.max(np.where(bound > 0, err / safe, np.where(err > 0, np.inf, 0.0))))


# ---- the packing, restated ---------------------------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "ctile tile_g tile lane")  # ctile[c] .. ctile[c + 1]: the tiles of colour c; (tile, lane) of every slot


def predicted_plan(blocks, colors, order=WIDTHS) -> Plan:
    """`order`: the width groups of a colour in this order (the library's is WIDTHS; anything else is a negative control)"""
    colors = np.asarray(colors, np.int64)
    nc = int(colors.max()) + 1 if len(colors) else 0
    off = slot_offsets(blocks)
    groups = {}
    for p, P in enumerate(blocks):
        groups.setdefault((int(colors[p]), padded_width(len(P))), []).append(p)
    ctile, tile_g = [0], []
    tile, lane = np.zeros(int(off[-1]), np.int64), np.zeros(int(off[-1]), np.int64)
    for c in range(nc):
        for g in order:
            per, group = 64 // g, groups.get((c, g), [])
            for k, p in enumerate(group):
                s = slice(int(off[p]), int(off[p + 1]))
                tile[s] = len(tile_g) + k // per
                lane[s] = (k % per) * g + np.arange(len(blocks[p]))
            tile_g += [g] * -(-len(group) // per)
        ctile.append(len(tile_g))
    return Plan(np.array(ctile, np.int64), np.array(tile_g, np.int64), tile, lane)


def check_plan(plan: Plan, blocks, colors) -> list:
    """what `plan` breaks of the packing rule, property by property (not by building the plan again); [] for the library's plan"""
    colors = np.asarray(colors, np.int64)
    off = slot_offsets(blocks)
    bad = []
    where = plan.tile * 64 + plan.lane
    if len(np.unique(where)) != len(where) or (plan.lane < 0).any() or (plan.lane >= 64).any():
        bad.append("a lane serves two slots")
    last = {}
    for p, P in enumerate(blocks):
        s0, m, c = int(off[p]), len(P), int(colors[p])
        t, l0, g = int(plan.tile[s0]), int(plan.lane[s0]), padded_width(len(P))
        if not (plan.tile[s0 : s0 + m] == t).all() or not np.array_equal(plan.lane[s0 : s0 + m], l0 + np.arange(m)) or l0 % g:
            bad.append(f"block {p} is not one run of lanes from a multiple of its width")
        if not plan.ctile[c] <= t < plan.ctile[c + 1]:
            bad.append(f"block {p} is outside the tiles of its colour")
        elif plan.tile_g[t] != g:
            bad.append(f"block {p} is in a tile of another width")
        # the blocks of a (colour, width) group fill their tiles densely in block order
        seen = last.get((c, g))
        if seen is None and l0:
            bad.append(f"block {p}, the first of its group, does not start a tile")
        if seen is not None and (t, l0) != ((seen[0], seen[1] + g) if seen[1] + g < 64 else (seen[0] + 1, 0)):
            bad.append(f"block {p} does not follow the block before it in its group")
        last[(c, g)] = (t, l0)
    for c in range(len(plan.ctile) - 1):
        if (np.diff(plan.tile_g[plan.ctile[c] : plan.ctile[c + 1]]) < 0).any():
            bad.append(f"the widths of colour {c} do not ascend")
    if set(plan.tile.tolist()) != set(range(int(plan.ctile[-1]))):
        bad.append("a tile holds no block")
    return bad


def tiles_per_color(plan: Plan):
    return tuple(int(v) for v in np.diff(plan.ctile))


def last_tile_blocks(plan: Plan, blocks, colors, c: int, g: int) -> int:
    """blocks in the last tile of the width-g group of colour c"""
    off = slot_offsets(blocks)
    t = [int(plan.tile[off[p]]) for p in range(len(blocks)) if colors[p] == c and padded_width(len(blocks[p])) == g]
    return t.count(max(t))


# ---- the launch maps, restated -----------------------------------------------------------------------------------------------------
def single_grid(nt: int) -> int:
    return -(-nt // WAVES)


def single_home(tl: int):
    """(workgroup, wavefront) of tile tl of a colour"""
    return tl // WAVES, tl % WAVES


def single_served(nt: int, waves: int = WAVES):
    """what blockgibbs_color_kernel does with its grid: [(workgroup, wavefront, tile)] of the wavefronts that pass `tl < ntiles`,
    and the number of wavefronts that leave early"""
    served, idle = [], 0
    for wg in range(single_grid(nt)):
        for wv in range(WAVES):
            tl = wg * waves + wv
            if tl < nt:
                served.append((wg, wv, tl))
            else:
                idle += 1
    return served, idle


ChainsLaunch = namedtuple("ChainsLaunch", "nt band nchunks ny grid")


def chains_launch(nt: int, C: int, band: int | None = None) -> ChainsLaunch:
    """`band`: None for the library's ceil(nt / 8); anything else is a negative control"""
    nchunks = -(-C // CB)
    band = -(-nt // XCDS) if band is None else band
    ny = min(nchunks, max(1, MAX_GRID // (XCDS * band)))
    return ChainsLaunch(nt, band, nchunks, ny, XCDS * band * ny)


def chains_served(L: ChainsLaunch, wid: int):
    """the (tile, chunk) pairs workgroup `wid` serves: none if it leaves early, else its chunk and every ny-th after it"""
    xcd, k = wid % XCDS, wid // XCDS
    tl = xcd * L.band + k // L.ny
    if tl >= L.nt:
        return []
    return [(tl, chunk) for chunk in range(k % L.ny, L.nchunks, L.ny)]


def covered_once(pairs, nt: int, nchunks: int) -> bool:
    """every (tile, chunk) of the launch exactly once, nothing else"""
    return sorted(pairs) == [(t, c) for t in range(nt) for c in range(nchunks)]


def chains_cover(L: ChainsLaunch) -> bool:
    return covered_once([tc for wid in range(L.grid) for tc in chains_served(L, wid)], L.nt, L.nchunks)


def idle_workgroups(L: ChainsLaunch) -> int:
    return sum(1 for wid in range(L.grid) if not chains_served(L, wid))


def idle_xcds(L: ChainsLaunch) -> int:
    """XCDs none of whose workgroups serves a tile"""
    busy = {wid % XCDS for wid in range(L.grid) if chains_served(L, wid)}
    return XCDS - len(busy)


# ---- operators and cases -----------------------------------------------------------------------------------------------------------
def banded_sparse(n: int, half_bandwidth: int, seed: int) -> O.CSR:
    """blockgibbs_cases.banded (symmetric, every entry within the band stored, strictly diagonally dominant with a positive diagonal:
    SPD) on the same draws, assembled from its diagonals"""
    rng = np.random.default_rng(seed)
    diags, offs, dom = [], [], np.zeros(n)
    for d in range(1, half_bandwidth + 1):
        v = -rng.uniform(0.1, 1.0, n - d)
        diags += [v, v]
        offs += [d, -d]
        dom[: n - d] += np.abs(v)
        dom[d:] += np.abs(v)
    return O.CSR.from_scipy(sp.diags([dom + 1.0] + diags, [0] + offs, shape=(n, n), format="csr"))


Case = namedtuple("Case", "name A blocks colors layout twin")  # colors None: first-fit; twin: a colouring of at most 2 tiles per colour

NAMES = ["gap-g8", "gap-g16", "gap-g32", "gap-g64", "gap-mixed", "wide-band", "ex6-33-stars"]
GAP_NAMES = NAMES[:5]
TILES = {**{f"gap-g{g}": TARGET_TILES for g in WIDTHS}, "gap-mixed": tuple(sum(t) for t in MIXED_TILES), "wide-band": (17, 17, 17, 17), "ex6-33-stars": (19, 18, 18, 18, 16, 16, 16, 16, 1)}


def _size_range(g: int):
    """the block sizes of width class g"""
    return (1 if g == 8 else g // 2 + 1), g


def _gapped(sizes):
    """consecutive blocks one gap row apart, and n: one further row behind the last block"""
    blocks, row = [], 0
    for m in sizes:
        blocks += consecutive_blocks([int(m)], row)
        row += int(m) + 1
    return blocks, row


def gap_last_fill(g: int, c: int) -> int:
    """blocks in the last tile of colour c of gap-g<g>"""
    return 1 + c % (64 // g)


def mixed_last_fill(g: int, c: int) -> int:
    """blocks in the last tile of the width-g group of colour c of gap-mixed: fewer than 64 / g wherever a tile takes several"""
    per = 64 // g
    return 1 + c % (per - 1) if per > 1 else 1


def _gap_case(g: int) -> Case:
    per, (lo, hi) = 64 // g, _size_range(g)
    counts = [(T - 1) * per + gap_last_fill(g, c) for c, T in enumerate(TARGET_TILES)]
    nb = sum(counts)
    # the colours in a random order over the blocks: a colour's tiles gather rows from all over the vector
    colors = np.random.default_rng(100 + g).permutation(np.repeat(np.arange(len(counts)), counts))
    blocks, n = _gapped(lo + np.arange(nb) % (hi - lo + 1))
    return Case(f"gap-g{g}", banded_sparse(n, 1, 20 + g), blocks, colors, None, np.arange(nb) // (2 * per))


def _mixed_case() -> Case:
    kinds = []  # (colour, width) of every block
    for c, tiles in enumerate(MIXED_TILES):
        for g, T in zip(WIDTHS, tiles):
            kinds += [(c, g)] * ((T - 1) * (64 // g) + mixed_last_fill(g, c))
    kinds = [kinds[i] for i in np.random.default_rng(7).permutation(len(kinds))]
    sizes, count = [], {}
    for c, g in kinds:
        lo, hi = _size_range(g)
        k = count[g] = count.get(g, -1) + 1
        sizes.append(lo + k % (hi - lo + 1))
    blocks, n = _gapped(sizes)
    return Case("gap-mixed", banded_sparse(n, 1, 19), blocks, np.array([c for c, _ in kinds]), None, np.arange(len(kinds)) // 2)


def _wide_case() -> Case:
    sizes = [4 + (3 * i) % 5 for i in range(532)]
    return Case("wide-band", banded_sparse(sum(sizes), 11, 23), consecutive_blocks(sizes), np.arange(532) % 4, None, None)


def _ex6_case() -> Case:
    A = O.ex6_matrix(33, 0.05)
    pos = np.random.default_rng(33).permutation(A.n + 37)[: A.n]
    return Case("ex6-33-stars", A, star_blocks(A), None, (A.n + 37, pos), None)


_built = {}


def case(name: str) -> Case:
    if name not in _built:
        _built[name] = _gap_case(int(name[5:])) if name[:5] == "gap-g" else {"gap-mixed": _mixed_case, "wide-band": _wide_case, "ex6-33-stars": _ex6_case}[name]()
    return _built[name]


def layout_of(c: Case):
    """(ld, pos) of the case's vectors"""
    return (c.A.n, np.arange(c.A.n)) if c.layout is None else (int(c.layout[0]), np.asarray(c.layout[1]))


def untouched_positions(c: Case):
    """rows in no block and layout padding"""
    ld, pos = layout_of(c)
    return np.setdiff1d(np.arange(ld), pos[np.unique(np.concatenate(c.blocks))])


def block_matrix(S: sp.csr_matrix, P):
    """A_PP as dpotrf('L') reads it (the lower triangle mirrored), dense m x m"""
    App = np.tril(S[P][:, P].toarray())
    return App + np.tril(App, -1).T


def numpy_factors(A: O.CSR, blocks):
    """numpy's own W = inv(cholesky(A_PP)) and kappa_2(A_PP) per block"""
    Ws, kappas, S = [], [], A.scipy()
    for P in blocks:
        App = block_matrix(S, np.asarray(P))
        Ws.append(sla.solve_triangular(np.linalg.cholesky(App), np.eye(len(P)), lower=True))
        w = np.linalg.eigvalsh(App)
        kappas.append(float(w[-1] / w[0]))
    return Ws, kappas


# ---- the walk-through, cached ------------------------------------------------------------------------------------------------------
class Walk:
    """blockgibbs_cases.walk_sweep on one (operator, blocks, W, layout): M = gram(W) and every block's exterior entries (value,
    position of the column, in storage order) are formed once.  A sweep runs the operations of walk_sweep on the same numbers
    in the same order -- the rows of a block side by side, which changes no rounding -- so it has its bits."""

    def __init__(self, A: O.CSR, blocks, Ws, pos=None):
        pos = np.arange(A.n) if pos is None else np.asarray(pos)
        self.blocks, self.Ws, self.off = blocks, Ws, slot_offsets(blocks)
        self.Ms = [gram(W) for W in Ws]
        self.P, self.ext = [], []
        rp, ci, va = A.rowptr, A.colidx, A.vals
        for P in blocks:
            P = np.asarray(P)
            rows = []
            for row in P:
                k = np.arange(rp[row], rp[row + 1])
                k = k[~np.isin(ci[k], P)]
                rows.append((va[k], pos[ci[k]]))
            w = max(len(v) for v, _ in rows)
            ev, ec, el = np.zeros((len(P), w)), np.zeros((len(P), w), np.int64), np.array([len(v) for v, _ in rows])
            for i, (v, cpos) in enumerate(rows):
                ev[i, : len(v)], ec[i, : len(v)] = v, cpos
            self.P.append(pos[P])
            self.ext.append((ev, ec, el))

    def sweep(self, colors, b, y, xi_slots=None, backward=False):
        y = np.array(y, np.float64, copy=True)
        for p in visit_order(colors, backward):
            P, W, M, (ev, ec, el) = self.P[p], self.Ws[p], self.Ms[p], self.ext[p]
            m = len(P)
            r = b[P].copy()
            for j in range(ev.shape[1]):
                on = el > j
                r[on] = r[on] - ev[on, j] * y[ec[on, j]]
            out = np.zeros(m)
            for j in range(m):
                out = out + M[:, j] * r[j]
            if xi_slots is not None:
                xi, acc = xi_slots[self.off[p] : self.off[p + 1]], np.zeros(m)
                for j in range(m):
                    acc = acc + W[j, :] * xi[j]
                out = out + acc
            y[P] = out
        return y

    def apply(self, colors, b, y, sweep_type, xi_fn=None):
        for d, dr in enumerate(directions(sweep_type)):
            y = self.sweep(colors, b, y, None if xi_fn is None else xi_fn(d), dr == BWD)
        return y

    def nnz_ext(self) -> int:
        return int(sum(el.sum() for _, _, el in self.ext))

    def independent_noise_bound(self, ld, tol, y_scale, b_scale, xi_scale):
        """blockgibbs_cases.noise_bound for ONE directional sweep over blocks that read no row another block writes: nothing
        propagates, so position by position it is (|W^T| 1) tol, the normals within `tol` of each other, plus noise_bound's `unit`
        term, 2 gamma(m + row length + 2) (||M||_inf (b_scale + ||A_ext||_inf y_scale) + ||W^T||_inf xi_scale)"""
        e = np.zeros(ld)
        for P, W, M, (ev, ec, el) in zip(self.P, self.Ws, self.Ms, self.ext):
            unit = 2 * gamma(len(P) + int(el.max()) + 2) * (np.abs(M).sum(axis=1).max() * (b_scale + np.abs(ev).sum(axis=1).max() * y_scale) + np.abs(W.T).sum(axis=1).max() * xi_scale)
            e[P] = np.abs(W.T).sum(axis=1) * tol + unit
        return e


def predicted_bytes(plan: Plan, nnz_ext: int, nslots: int) -> float:
    """pmg_blockgibbs_get_algorithmic_bytes from the restated plan: it holds the library's sum of tile widths to the prediction"""
    return 2.0 * 8.0 * 64.0 * float(plan.tile_g.sum()) + 12.0 * nnz_ext + 28.0 * nslots
