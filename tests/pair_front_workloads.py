"""Child process of test_gpu_grid_pair_front.py: noisy red-black chains and plane-range launches on the shapes at which the
row addressing of grid_color_pair_sweep_kernel can go wrong, in a fresh process (the PMG_* switches are read once per
process); natural-order float64 vectors written to an .npz.  The parent imports the shapes and the inputs from here.

    python pair_front_workloads.py <out.npz>
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent

# one and two x blocks; south and north clamps on one line, on alternating lines, and lines in a second workgroup; both z
# faces in one pair, an odd last pair, the down and the up clamp in different pairs
SHAPES = [(nx, ny, nz) for nx in (256, 512) for ny in (1, 2, 8, 9) for nz in (2, 3, 4, 5)]
KAPPA, SEED, COUNTER0, SWEEPS = 1.5, (1 << 40) + 0xF00D, 2, 3
# plane ranges of nz = 5: (kbegin, kcount, noise counter), both colours each
RANGE_SHAPES = [(256, 9, 5), (512, 2, 5)]
RANGES = [(1, 3, 7), (2, 1, 8)]
# a slab: planes 1 .. 4 of five (an odd first plane, a ghost plane below, the domain's top face above); the whole slab, then
# the ranges
SLAB = (256, 9, 5, 1, 4)
SLAB_RANGES = [(0, 4, 5), (1, 3, 7), (2, 1, 8)]


def inputs(nx, ny, nz):
    """(b, y0) of a shape, natural order"""
    rng = np.random.default_rng(nx * 1000 + ny * 10 + nz)
    return rng.standard_normal(nx * ny * nz), rng.standard_normal(nx * ny * nz)


def main(path):
    sys.path.insert(0, str(ROOT))
    import torch

    from parmgmc_amd import GridMCSOR

    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")
    out = {}
    for nx, ny, nz in SHAPES:
        b, y0 = inputs(nx, ny, nz)
        g = GridMCSOR(nx, ny, nz, KAPPA)
        g.set_omega(1.0)
        y = dev(y0)
        g.sample(dev(b), y, SWEEPS, seed=SEED, counter0=COUNTER0)
        out[f"chain/{nx}x{ny}x{nz}"] = y.cpu().numpy()
        if (nx, ny, nz) in RANGE_SHAPES:
            bc, yc = g.to_cvec(dev(b)), g.to_cvec(dev(y0))
            for kbegin, kcount, ctr in RANGES:
                for c in (0, 1):
                    g.sweep_color_planes_cvec(c, kbegin, kcount, bc, yc, noisy=True, seed=SEED, counter=ctr)
                out[f"range/{nx}x{ny}x{nz}/k{kbegin}+{kcount}"] = g.from_cvec(yc).cpu().numpy()
        g.destroy()
    # the slab: its lower ghost plane is the owned plane of a one-plane slab below it
    nx, ny, nzg, kz0, nzo = SLAB
    b, y0 = inputs(nx, ny, nzg)
    plane = nx * ny
    g, below = GridMCSOR(nx, ny, nzg, KAPPA, kz0=kz0, nz_owned=nzo), GridMCSOR(nx, ny, nzg, KAPPA, kz0=kz0 - 1, nz_owned=1)
    g.set_omega(1.0)
    bc, yc = g.to_cvec(dev(b[kz0 * plane:(kz0 + nzo) * plane])), g.to_cvec(dev(y0[kz0 * plane:(kz0 + nzo) * plane]))
    yb = below.to_cvec(dev(y0[(kz0 - 1) * plane:kz0 * plane]))
    for c in (0, 1):
        own, _, n = below.halo_plane(c, 1)
        _, ghost, _ = g.halo_plane(c, 0)
        yc[ghost:ghost + n].copy_(yb[own:own + n])
    for kbegin, kcount, ctr in SLAB_RANGES:
        for c in (0, 1):
            g.sweep_color_planes_cvec(c, kbegin, kcount, bc, yc, noisy=True, seed=SEED, counter=ctr)
        out[f"slab/k{kbegin}+{kcount}"] = g.from_cvec(yc).cpu().numpy()
    g.destroy()
    below.destroy()
    torch.cuda.synchronize()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
