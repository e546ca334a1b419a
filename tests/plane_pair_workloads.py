"""Child process of test_gpu_grid_plane_pair.py: red-black grid chains on one group of shapes in a fresh process (the PMG_*
switches are read once per process), raw float64 colour vectors written to an .npz.

    python plane_pair_workloads.py <group> <out.npz>
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent

# (nx, ny, nz): what the pairing can get wrong there.  The parent runs this group with lines neither packed into wavefronts
# nor tail-collected, so that every shape is on the plain one-line-per-wavefront mapping.
PLAIN_SHAPES = [
    (8, 4, 1),      # a lone plane with no partner
    (8, 4, 2),      # one pair, both z faces
    (6, 5, 3),      # odd nz, odd ny, nx not a multiple of 4
    (130, 9, 5),    # a line end inside the wavefront, an odd line count
    (258, 8, 4),    # a pad slot at the line end, a second wavefront per line with one live lane
    (512, 8, 6),    # the headline line length, full wavefronts
    (9, 5, 4),      # odd nx: the last lane has a point on one plane of each pair only
]
# under the default switches: the plain mapping without help, XCD bands of whole line tiles (what 512^3 selects), the flat
# walk over bands of 7 lines with one more in six of them and an odd number of planes, two wavefronts per line; and a
# tail-mapped shape, which keeps the one-plane kernel
DEFAULT_SHAPES = [(512, 8, 6), (170, 64, 4), (170, 62, 5), (400, 62, 4), (257, 257, 4)]
GROUPS = {"plain": PLAIN_SHAPES, "default": DEFAULT_SHAPES}
# a slab of a taller grid (planes 3 .. 7 of 9): parities come from the global plane, pairs from the launch-local index
SLAB = (170, 6, 9, 3, 5)
SEED_BIG = (1 << 40) + 0xBEEF  # above 2^32


def main(group, path):
    sys.path.insert(0, str(ROOT))
    import torch

    from parmgmc_amd import GridMCSOR

    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")
    out = {}
    for nx, ny, nz in GROUPS[group]:
        n = nx * ny * nz
        rng = np.random.default_rng(n)
        b, y0 = rng.standard_normal(n), rng.standard_normal(n)
        g = GridMCSOR(nx, ny, nz, 1.5)
        bc = g.to_cvec(dev(b))
        for om in (1.0, 1.3):
            g.set_omega(om)
            for t in (1, 2, 3):  # forward, backward, symmetric
                g.set_sweep_type(t)
                y = g.to_cvec(dev(y0))
                g.sample_cvec(bc, y, 3, SEED_BIG, 1)
                out[f"{nx}x{ny}x{nz}/om{om}/t{t}/noisy"] = y.cpu().numpy()
                y = g.to_cvec(dev(y0))
                for _ in range(3):
                    g.apply_cvec(bc, y)
                out[f"{nx}x{ny}x{nz}/om{om}/t{t}/det"] = y.cpu().numpy()
        g.destroy()
    if group == "default":
        nx, ny, nzg, kz0, nzo = SLAB
        n = nx * ny * nzo
        rng = np.random.default_rng(n)
        g = GridMCSOR(nx, ny, nzg, 1.5, kz0=kz0, nz_owned=nzo)
        bc = g.to_cvec(dev(rng.standard_normal(n)))
        y = dev(rng.standard_normal(g.cvec_len))  # ghost planes included: the slab's neighbours
        for kbegin, kcount in ((0, nzo), (1, 3), (1, 4), (4, 1)):
            for c in (0, 1):
                g.sweep_color_planes_cvec(c, kbegin, kcount, bc, y, noisy=True, seed=SEED_BIG, counter=7)
                g.sweep_color_planes_cvec(c, kbegin, kcount, bc, y)
            out[f"slab/k{kbegin}+{kcount}"] = y.cpu().numpy()
        g.destroy()
    torch.cuda.synchronize()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
