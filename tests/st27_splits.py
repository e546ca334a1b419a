"""How the paired class-stencil kernels cut a level into wavefronts, restated in Python (split_pairs, xcd_grid, launch_phase and
pmgk_st27_residual_pair in kernels_stencil27_pair.hip, the plane-kernel rule of pmgk_st27_sweep_phase in kernels_stencil27.hip),
and the class-stencil level shapes the suite uses to reach every branch of that rule.

A thread owns a PAIR of points of a line, a line of nx points has npairs = (nx + 1) / 2 of them.  A wavefront holds `valid`
pairs whose results are final plus `halo` lanes on either side (sweep: 60 + 2 x 2, residual: 62 + 2 x 1).  split_pairs cuts a
line into full segments and a remainder; a remainder narrow enough for two or more to share a wavefront (segw = rem + 2 halo
<= 32) is swept by a second, PACKED launch that holds the remainders of nseg = 64 / segw lines side by side.  Lines fall into
tiles of 2 PT = 8 (sweep: PT + 1 first-stage lines, PT second-stage lines per workgroup) or 4 (residual) lines; the packed
sweep takes its nseg lines from nseg consecutive line TILES, the packed residual from nseg consecutive lines.

test_st27_splits.py checks the table against the restatement and the restatement's constants against the .hip sources without a
GPU; test_gpu_st27_splits.py runs every shape against the oracle and checks the restated launches against the kernel trace.  A
shape that slides back to a 2^k + 1 extent fails there, not silently."""
from collections import namedtuple

PT = 4            # line pairs per sweep tile
SWEEP = (60, 2)   # (VALID, HL) of the sweep
RESID = (62, 1)   # valid pairs and halo lanes of the residual
RESID_TILE = 4    # lines per residual workgroup
PLANE_LIMIT = 1100  # points per plane up to which the per-colour path (PMG_ST27_PAIR=0) takes the one-workgroup-per-plane kernel

Split = namedtuple("Split", "nbx_main p0 segw nseg rem")
Split.packed = property(lambda s: s.p0 >= 0)


def split_pairs(npairs, valid, halo, pack=True):
    """nbx_main full-width segments of the one-line-per-wavefront launch; p0 the first pair of the packed remainder (-1: none),
    its segment width and the segments per wavefront; rem: the pairs of the last segment, packed or not"""
    nbx = (npairs + valid - 1) // valid
    rem = npairs - valid * (nbx - 1)
    segw = rem + 2 * halo
    if pack and 64 // segw >= 2:
        return Split(nbx - 1, valid * (nbx - 1), segw, 64 // segw, rem)
    return Split(nbx, -1, 0, 0, rem)


def xcd_grid(nbx, nby, nbz):
    """workgroups of a launch whose (line tile, plane) items are dealt in eighths to the XCDs: padded to a multiple of 8"""
    return 8 * nbx * ((nby * nbz + 7) // 8)


def sweep_split(cx, pack=True):
    return split_pairs((cx + 1) // 2, *SWEEP, pack=pack)


def residual_split(cx, pack=True):
    return split_pairs((cx + 1) // 2, *RESID, pack=pack)


def phase_planes(cz):
    """planes of z-parity 0 and 1"""
    return [(cz - pz + 1) // 2 for pz in (0, 1)]


def sweep_launches(cx, cy, cz, pack=True):
    """(packed?, workgroups) of every launch of one directional sweep; a workgroup has 64 x (PT + 1) threads"""
    P, nby, out = sweep_split(cx, pack), (cy + 2 * PT - 1) // (2 * PT), []
    for planes in phase_planes(cz):
        if planes <= 0:
            continue
        if P.nbx_main > 0:
            out.append((False, xcd_grid(P.nbx_main, nby, planes)))
        if P.packed:
            out.append((True, xcd_grid(1, (nby + P.nseg - 1) // P.nseg, planes)))
    return out


def residual_launches(cx, cy, cz, pack=True):
    """(packed?, workgroups) of the residual's launches; a workgroup has 64 x 4 threads"""
    P, out = residual_split(cx, pack), []
    if P.nbx_main > 0:
        out.append((False, xcd_grid(P.nbx_main, (cy + RESID_TILE - 1) // RESID_TILE, cz)))
    if P.packed:
        out.append((True, xcd_grid(1, (cy + RESID_TILE * P.nseg - 1) // (RESID_TILE * P.nseg), cz)))
    return out


def sweep_idle_segments(cx, cy):
    """segments of the last packed sweep workgroup of a plane that have no line tile"""
    P, nby = sweep_split(cx), (cy + 2 * PT - 1) // (2 * PT)
    return (nby + P.nseg - 1) // P.nseg * P.nseg - nby if P.packed else 0


def residual_idle_lines(cx, cy):
    """(wavefront, segment) slots of the last packed residual workgroup of a plane that have no line"""
    P = residual_split(cx)
    per = RESID_TILE * P.nseg
    return (cy + per - 1) // per * per - cy if P.packed else 0


def plane_kernel(cx, cy, limit=PLANE_LIMIT):
    """PMG_ST27_PAIR=0: one workgroup of 1024 threads sweeps a plane (True) or one launch per colour (False)"""
    return cx * cy <= limit


def plane_launches(cx, cy, cz):
    """workgroups (of 1024 threads) of the plane kernel's launches of one directional sweep: one per z-parity phase with planes"""
    return [p for p in phase_planes(cz) if p > 0]


def color_launches(cx, cy, cz):
    """(workgroups of 256 threads, planes) of the per-colour kernel's launches of one directional sweep: the colours with points"""
    out = []
    for col in range(8):
        n = [(d - ((col >> a) & 1) + 1) // 2 for a, d in enumerate((cx, cy, cz))]
        if min(n) > 0:
            out.append(((n[0] * n[1] + 255) // 256, n[2]))
    return out


def kind(P, valid):
    """the branch of split_pairs a line takes"""
    if P.packed:
        return "packed behind main" if P.nbx_main else "all packed"
    if P.nbx_main == 1:
        return "one full" if P.rem == valid else "one partial"
    return "full segments" if P.rem == valid else "unpacked behind main"


def fine_grid(shape):
    """the DMDA grid whose first coarse level is the class-stencil level `shape` (2c - 1 points; one plane stays one plane)"""
    cx, cy, cz = shape
    return (2 * cx - 1, 2 * cy - 1, 2 * cz - 1 if cz > 1 else 1)


def coarsen(dims):
    return tuple((d - 1) // 2 + 1 if d > 1 else 1 for d in dims)


# class-stencil level (cx, cy, cz) -> (sweep branch, residual branch, what it is there for)
SHAPES = {
    (55, 8, 2): ("all packed", "all packed", "28 pairs: the widest packed sweep segment (segw 32, nseg 2), residual segw 30; one full line tile, even line count"),
    (57, 9, 3): ("one partial", "all packed", "29 pairs: the first unpacked sweep remainder; residual segw 31"),
    (59, 7, 1): ("one partial", "all packed", "30 pairs: residual segw 32, the widest packed; a 2-D level, where the odd z phase has no plane"),
    (61, 18, 2): ("one partial", "one partial", "31 pairs: the first unpacked residual remainder; planes of 1098 points, beyond 1024 threads of the plane kernel"),
    (119, 3, 2): ("one full", "one partial", "exactly 60 pairs, odd nx: the last valid lane is the line's last pair, with one point"),
    (120, 4, 2): ("one full", "one partial", "exactly 60 pairs, even nx"),
    (121, 17, 3): ("packed behind main", "one partial", "61 pairs: sweep remainder 1 (segw 5, nseg 12), 3 line tiles so 9 segments idle; residual 61 of 62"),
    (123, 5, 2): ("packed behind main", "one full", "62 pairs: the residual's full segment; sweep remainder 2"),
    (125, 12, 2): ("packed behind main", "packed behind main", "63 pairs: residual remainder 1 (segw 3, nseg 21); a 4-line tile behind a full one"),
    (175, 16, 2): ("packed behind main", "packed behind main", "88 pairs: sweep remainder 28 packed behind a main segment; two full line tiles"),
    (177, 10, 3): ("unpacked behind main", "packed behind main", "89 pairs: sweep remainder 29 unpacked behind a main segment, a seam between two wavefronts"),
    (183, 6, 2): ("unpacked behind main", "packed behind main", "92 pairs: residual remainder 30, the widest packed one (segw 32, nseg 2), behind a main segment; six lines"),
    (185, 11, 2): ("unpacked behind main", "unpacked behind main", "93 pairs: residual remainder 31, the first unpacked one, behind a main segment; 11 lines"),
    (199, 15, 4): ("unpacked behind main", "unpacked behind main", "100 pairs = 60 + 40: a full and a partial wavefront, the Box-Muller draw handed across the seam; even cz"),
    (239, 14, 2): ("full segments", "unpacked behind main", "120 pairs: two full sweep segments"),
    (241, 9, 2): ("packed behind main", "unpacked behind main", "121 pairs: remainder 1 behind two sweep segments"),
    (247, 13, 2): ("packed behind main", "full segments", "124 pairs: two full residual segments; 13 lines"),
}
assert all(cx * cy * cz <= 17_000 for cx, cy, cz in SHAPES)  # the suite's levels stay small

# line lengths and line counts of the class-stencil levels that test_gpu_vcycle_shapes_oracle.py, test_gpu_fullsize_oracle.py,
# test_gpu_fused_rr.py and switch_workloads.py reach: what the suite ran before this table
SUITE_NX = (2, 3, 5, 9, 17, 33, 65, 129, 144, 257)


def suite_ny_before(cy):
    """was a class-stencil line count like cy in the suite before this table?"""
    return cy <= 5 or cy % 8 == 1


# hierarchies run beside the table: (fine grid, levels) -> what for
THREE_LEVEL = ((481, 33, 9), 3)   # (241, 17, 5) -> (121, 9, 3): st27_restrict_full_kernel, st27_prolong_add_cell_kernel between class-stencil levels
SEMICOARSENED = ((241, 33, 1), 2)  # z never coarsens: the generic Q1 transfers
FLAT_QUAD = ((513, 257, 3), 2)    # q1_prolong_add_quad_kernel in its `runs` form: nb = 66 >= 64 quads per line, padded to 72
# whole V-cycles of three levels: fine grid -> levels.  The first coarse level is a class-stencil level with a tabled line length,
# the coarsest the Cholesky (or Gibbs) level.  A level can only be coarsened again if its extents are odd (2 c - 1 points), so
# (177, 10, 3) and (199, 15, 4) are stood in for by (177, 11, 3) and (199, 11, 3): the same lines, odd line and plane counts
# (and a coarsest level of 1200 points, which the oracle's dense Cholesky factor still takes in under a second).
VCYCLE_LEVELS = [(57, 9, 3), (121, 17, 3), (177, 11, 3), (199, 11, 3)]
VCYCLE_SHAPES = {fine_grid(s): 3 for s in VCYCLE_LEVELS}


def quad_prolong_blocks(nx, ny):
    """q1_prolong_add_quad_kernel (pmgk_q1_prolong_add in kernels_transfer.hip): blocks of 256 threads per plane pair and colour,
    a thread per pair of fine lines and red-black column; from 64 blocks on the launch is padded to a multiple of 8 and every XCD
    takes a contiguous run of them.  Returns (blocks needed, blocks launched)."""
    tplE = ((nx + 1) // 2 + 1) // 2
    nb = ((ny + 1) // 2 * tplE + 255) // 256
    return nb, (nb + 7) // 8 * 8 if nb >= 64 else nb


def st27_levels(grid, levels, coarse_gibbs):
    """dims of the class-stencil levels of MGMC(*grid, kappa, levels): every level below the grid level, the coarsest only
    when it is sampled by Gibbs sweeps"""
    dims, out = grid, []
    for l in range(levels - 2, -1, -1):
        dims = coarsen(dims)
        if l > 0 or coarse_gibbs:
            out.append(dims)
    return out
