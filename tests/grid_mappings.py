"""The thread mapping of the red-black grid sweep, restated in Python (grid_choose_mapping in kernels_grid.hip), and the
shapes the suite uses to reach each of its branches.

grid_color_sweep_kernel deals the threads of one colour pass to the wavefronts in one of several ways, chosen from
(nx, ny) alone:
  packed  lines packed into wavefronts without gaps;
  plain   one line per wavefront, grid (line tiles of 64 threads, tiles of 4 lines, planes);
  tail    full wavefronts per line, the few threads left over per line collected behind the last plane;
  banded  >= 16 line tiles: XCD-banded dispatch, eight bands of ceil(ny / 8) lines with a clamped last band;
  flat    bands that are not whole line tiles: a flat (plane, line) walk over bands of floor(ny / 8) lines, the
          ny mod 8 lines left over going one each to the last bands.
The in-kernel halo hand-shake (transport "ipc") switches tail and flat off, so the same shape lands on another branch.

Every table below states, per shape, the branch of the single-device rule and of the halo rule; test_grid_mappings.py
checks the tables against the restatement without a GPU, and test_gpu_switches.py checks the restatement against the
kernel trace.  A shape list that slides back to packed fails there, not silently."""
from collections import namedtuple

Mapping = namedtuple("Mapping", "tail packed banded flat gsize remainder waves bandw")
Mapping.flags = property(lambda m: dict(tail=m.tail, packed=m.packed, banded=m.banded, flat=m.flat))


def sweep_mapping(nx, ny, nz, halo=False):
    """The host's choice for a grid sweep over nz planes (grid_choose_mapping in kernels_grid.hip, default switches, the
    tightest line stride of grids that fit the Infinity Cache); halo: the rule of the in-kernel halo hand-shake, no tail
    and no flat.  Flags, the launch's grid size in work-items, the band remainder ny - 8 (ny // 8), the wavefronts per line
    of the one-line-per-wavefront mappings (0: packed) and the lines per XCD band as the launch uses them (0: not banded)."""
    half = (nx + 1) // 2
    sx = (half + 1) // 2 * 2
    tpl, tplE, nby = sx // 2, (half + 1) // 2, (ny + 3) // 4
    tmain = tplE // 64 * 64
    tailw = tplE - tmain
    tail = not halo and tmain > 0 and 0 < tailw <= 8
    packed = not tail and 2 * ((tpl + 63) // 64 * 64) >= 3 * tplE
    nbx = tplE if packed else (tmain // 64 if tail else (tpl + 63) // 64)
    bandw = (ny + 7) // 8 if (not packed and nby >= 16) else 0
    banded, flat = bandw > 0, False
    if packed:
        grid = ((ny * tplE + 255) // 256, 1, nz)
    else:
        gx, gy = (8 * nbx, (bandw + 3) // 4) if bandw else (nbx, nby)
        zl = nz
        if not halo and bandw and ((bandw & 3) or 8 * bandw != ny):
            flat = True
            bandw = ny // 8
            maxband = bandw + (1 if ny > 8 * bandw else 0)
            zl = (maxband * nz + 4 * gy - 1) // (4 * gy)
        ztail = (nz * ((ny * tailw + 255) // 256) + gx * gy - 1) // (gx * gy) if tail else 0
        grid = (gx, gy, zl + ztail)
    return Mapping(tail, packed, banded, flat, (grid[0] * 64, grid[1] * 4, grid[2]), ny - 8 * (ny // 8), 0 if packed else nbx, bandw)


def _f(tail=False, packed=False, banded=False, flat=False):
    return dict(tail=tail, packed=packed, banded=banded, flat=flat)


PACKED, PLAIN, BANDED = _f(packed=True), _f(), _f(banded=True)
FLAT, TAIL, TAIL_FLAT = _f(banded=True, flat=True), _f(tail=True), _f(tail=True, banded=True, flat=True)

# (nx, ny, nz) -> (branch under the single-device rule, branch under the halo rule)

# single-device sweeps, residual and plane-range composition of test_gpu_grid.py (170 = 43 threads per line: one wavefront,
# two thirds full; 400 = 100 threads: two wavefronts; 513 = 129 threads: two full wavefronts + one tail thread)
UNPACKED_SHAPES = {
    (170, 6, 5): (PLAIN, PLAIN),          # two line tiles, the second with two lines
    (170, 64, 3): (BANDED, BANDED),       # sixteen line tiles, bands of 8 lines: whole tiles, no flat walk
    (400, 62, 3): (FLAT, BANDED),         # two wavefronts per line; bands of 7 lines, six of them with one more
    (513, 66, 2): (TAIL_FLAT, BANDED),    # bands of 8 lines + 2; under the halo rule three wavefronts per line, bands of 9
}

# test_xcd_bands_of_any_remainder_sweep_every_line_once: the flat walk at every remainder ny mod 8, at bands of 7 lines
# (ny = 61..63: five to seven bands take one line more) and of 8, 9, 16 and 32; ny = 64 and 72 are the whole-tile and the
# odd-band-width neighbours.  All with five planes.
BAND_SHAPES = {(170, ny, 5): (FLAT, BANDED) for ny in list(range(61, 74)) + [257]}
BAND_SHAPES[(170, 64, 5)] = (BANDED, BANDED)
BAND_SHAPES[(257, 129, 5)] = (TAIL_FLAT, PACKED)  # an x tail on top of the flat walk
# the same line counts at 3 threads per line: packed, where neither bands nor the flat walk exist -- controls
BAND_CONTROLS = {(12, ny, 5): (PACKED, PACKED) for ny in list(range(61, 73)) + [257]}

# slab layouts (kz0 != 0, plane ranges) without the halo hand-shake: SlabSet and the schedule of run_samples.  Six planes,
# cut so that kz0 is odd and even and one slab has a single plane.
SLAB_SHAPES = {
    (257, 5, 6): (TAIL, PACKED),          # compact tail: one tail thread per line, only the lines of this colour
    (261, 3, 6): (TAIL, PACKED),          # two tail threads per line
    (257, 66, 6): (TAIL_FLAT, PACKED),
    (170, 62, 6): (FLAT, BANDED),
    (170, 64, 6): (BANDED, BANDED),
    (400, 62, 6): (FLAT, BANDED),
}
SLAB_CUTS = ([0, 1, 4, 6], [0, 3, 6])

# the in-kernel halo kernel, one process (IpcSlabDriver loopback)
HALO_SHAPES = {
    (170, 18, 4): (PLAIN, PLAIN),         # unpacked, five line tiles, the last with two lines
    (170, 64, 3): (BANDED, BANDED),       # bands of 8 lines: whole line tiles
    (170, 61, 3): (FLAT, BANDED),         # bands of 8 lines, the last one with 5
    (170, 66, 2): (FLAT, BANDED),         # bands of 9 lines = three tiles with 4 + 4 + 1, the last band with 3
    (170, 66, 1): (FLAT, BANDED),         # one plane is both faces
    (513, 6, 4): (TAIL, PLAIN),           # three wavefronts per line, the third with one live lane
    (513, 66, 2): (TAIL_FLAT, BANDED),    # the same in bands of 9 lines
    (40, 18, 7): (PACKED, PACKED),        # control: what every halo launch of the suite used to be
}
# ranks sharing the GPU over ipc: (nx, ny, nz, world) -> branches; the slabs of 170 x 61 x 6 on 5 ranks have 2, 1, 1, 1, 1 planes
HALO_RANK_SHAPES = {
    (170, 66, 7, 3): (FLAT, BANDED),
    (170, 61, 6, 5): (FLAT, BANDED),
    (513, 66, 4, 2): (TAIL_FLAT, BANDED),
}
# grid level of the distributed V-cycles and of the oracle comparison that pins their single-device side
HALO_VCYCLE_SHAPES = {
    (513, 9, 9): (TAIL, PLAIN),
    (513, 65, 9): (TAIL_FLAT, BANDED),
}
# the packed neighbours of the tail shapes: under the halo rule 65 or 66 threads per line pack
HALO_PACKED_SHAPES = {
    (257, 66, 5): (TAIL_FLAT, PACKED),
    (261, 66, 3): (TAIL_FLAT, PACKED),
}

# part-A shape (grid level) of test_gpu_vcycle_shapes_oracle.py and the GridMCSOR-only shapes of switch_workloads.py -> the
# thread mapping of its single-device grid sweep, checked against the default child's kernel trace in test_gpu_switches.py:
# tail threads collected in blocks of their own (threads per line tplE >= 64, tplE % 64 <= 8), lines packed into wavefronts,
# XCD-banded dispatch (>= 16 line tiles), flat (plane, line) runs over the bands (bands that are not whole line tiles)
SHAPE_BRANCHES = {
    (257, 9, 9): TAIL,                    # tplE 65: 1 tail thread per line
    (287, 5, 5): TAIL,                    # tplE 72: 8 tail threads
    (257, 65, 9): TAIL_FLAT,              # 17 line tiles, bands of 9 lines
    (65, 65, 65): PACKED,
    (129, 65, 17): PACKED,
    (257, 257, 1): TAIL_FLAT,             # bands of 33 lines
    (9, 9, 129): PACKED,
    (33, 3, 33): PACKED,
    (5, 5, 5): PACKED,
    (255, 65, 3): FLAT,                  # GridMCSOR only from here on: the plain unpacked mapping
    (170, 62, 3): FLAT,                   # bands of 7 lines, six with one more
    (170, 64, 3): BANDED,                 # whole line tiles: banded, no flat walk
    (400, 62, 3): FLAT,                   # two wavefronts per line
}
# the loopback workload of switch_workloads.py: the halo kernel on the plain mapping, and the launch it must show
HALO_TRACE_SHAPE = (170, 66, 2)
HALO_TRACE_GSIZE = (512, 12, 2)

TABLES = {"UNPACKED_SHAPES": UNPACKED_SHAPES, "BAND_SHAPES": BAND_SHAPES, "BAND_CONTROLS": BAND_CONTROLS, "SLAB_SHAPES": SLAB_SHAPES,
          "HALO_SHAPES": HALO_SHAPES, "HALO_RANK_SHAPES": HALO_RANK_SHAPES, "HALO_VCYCLE_SHAPES": HALO_VCYCLE_SHAPES,
          "HALO_PACKED_SHAPES": HALO_PACKED_SHAPES}
