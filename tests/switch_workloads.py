"""Child process of test_gpu_switches.py: runs one fixed set of workloads in a fresh process (the PMG_* runtime switches
are read once per process, so every configuration needs a process of its own) and writes the raw float64 results to an
.npz -- single-device grid sweeps, one chain through the in-kernel halo kernel (ipc loopback), V-cycles, AIJ samplers.
Keys starting with "meta/" are layout facts that show a switch took effect (line strides, AIJ row layouts); all
other keys are results that must not change by a bit.

    python switch_workloads.py <out.npz> <config4.npz>
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent

# GridMCSOR.sample: part-A shapes, a tail-mapped, banded + flat grid, the plain one-line-per-wavefront mapping (255 = 4 x 64
# threads per line, no tail; 170 = 43 threads in one wavefront; 400 = 100 threads in two: flat over bands of 7 lines, banded
# by whole line tiles, flat with two wavefronts per line -- SHAPE_BRANCHES of grid_mappings.py) and TAIL_GRIDS of test_gpu_grid.py
GRID_SHAPES = [(257, 9, 9, 2.0), (287, 5, 5, 1.0), (255, 65, 3, 1.0), (65, 65, 5, 2.0),
               (257, 5, 3, 10.0), (261, 3, 2, 1.0), (287, 2, 1, 0.5), (513, 2, 2, 2.0), (257, 70, 2, 1.0),
               (170, 62, 3, 1.0), (170, 64, 3, 2.0), (400, 62, 3, 1.0)]
# the in-kernel halo kernel in this process (IpcSlabDriver loopback: the rank is its own z-neighbour): HALO_TRACE_SHAPE of
# grid_mappings.py, the plain mapping in XCD bands of 9 lines with a short last band
HALO_SHAPE = (170, 66, 2, 1.5)
GRID_SETTINGS = [(1.0, 1, True), (1.0, 2, False), (1.3, 3, True)]  # (omega, sweep type, scaled)

# MGMC.sample: the part-A shapes of test_gpu_vcycle_shapes_oracle.py, and one of 8.5 M points where the fused residual +
# restriction takes its one-barrier-per-plane form by default (PMG_GRID_RR_SYNC)
MG_SHAPES = [((257, 9, 9), 3), ((287, 5, 5), 2), ((257, 65, 9), 4), ((65, 65, 65), 4), ((129, 65, 17), 4),
             ((257, 257, 1), 5), ((9, 9, 129), 4), ((33, 3, 33), 2), ((5, 5, 5), 2)]
MG_BIG = ((257, 257, 129), 6)
# (scaled, omega, sweep, nu, coarse, coarse its, correction form)
MG_SETTINGS = {"fwd": (False, 1.0, 1, 1, "cholsampler", 1, False),
               "bwd": (False, 1.0, 2, 1, "cholsampler", 1, False),
               "mix": (True, 1.3, 3, 2, "gibbs", 2, True)}


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def _host(t):
    return t.detach().cpu().numpy().copy()


def grid_runs(out):
    from parmgmc_amd import GridMCSOR

    for nx, ny, nz, kappa in GRID_SHAPES:
        n = nx * ny * nz
        rng = np.random.default_rng(n)
        b, y0 = rng.standard_normal(n), rng.standard_normal(n)
        g = GridMCSOR(nx, ny, nz, kappa)
        out[f"meta/cvec/{nx}x{ny}x{nz}"] = np.array([g.new_cvec().numel()], np.float64)
        for om, t, scaled in GRID_SETTINGS:
            g.set_omega(om)
            g.set_sweep_type(t)
            y = _dev(y0)
            g.sample(_dev(b), y, 3, seed=0xBEEF, counter0=1, scaled=scaled)
            out[f"grid/{nx}x{ny}x{nz}/om{om}/t{t}"] = _host(y)
        g.destroy()


def halo_run(out):
    from parmgmc_amd import GridMCSOR
    from parmgmc_amd.dist import IpcSlabDriver

    nx, ny, nz, kappa = HALO_SHAPE
    n = nx * ny * nz
    rng = np.random.default_rng(n)
    b0, y0 = rng.standard_normal(n), rng.standard_normal(n)
    g = GridMCSOR(nx, ny, nz, kappa)
    drv = IpcSlabDriver(g, 0, 1, loopback=True)
    b = g.to_cvec(_dev(b0))
    for om, t, scaled in GRID_SETTINGS:
        g.set_omega(om)
        y = g.to_cvec(_dev(y0))
        drv.sample_cvec(b, y, 3, scaled, t, 0xBEEF, 1)
        out[f"halo/{nx}x{ny}x{nz}/om{om}/t{t}"] = _host(g.from_cvec(y))
    drv.destroy()
    g.destroy()


def mg_run(grid, levels, setting, its, guesszero=False):
    from parmgmc_amd import MGMC

    scaled, omega, sweep, nu, coarse, cits, literal = MG_SETTINGS[setting]
    n = int(np.prod(grid))
    rng = np.random.default_rng(n + levels)
    b, y0 = rng.standard_normal(n), rng.standard_normal(n)
    mg = MGMC(*grid, 1.5, levels)
    mg.set_smoother(scaled, omega, sweep, nu)
    mg.set_coarse(coarse, cits)
    mg.set_correction_form(literal)
    mg.setup()
    seen = []
    y = _dev(np.zeros(n) if guesszero else y0)
    mg.sample(_dev(b), y, its, seed=0xACE, counter0=3, guesszero=guesszero, callback=lambda it, yy: seen.append(_host(yy)))
    mg.destroy()
    return np.concatenate(seen)


def mg_runs(out):
    for grid, levels in MG_SHAPES:
        key = "x".join(map(str, grid))
        for s in MG_SETTINGS:
            out[f"mg/{key}/{s}"] = mg_run(grid, levels, s, 3)
        out[f"mg/{key}/guesszero"] = mg_run(grid, levels, "fwd", 2, guesszero=True)
    out["mg/big/fwd"] = mg_run(*MG_BIG, "fwd", 1)


def aij_runs(out, config4):
    import oracle as O
    from parmgmc_amd import COLORING_ITERATED, MCSOR, MGMC

    z = np.load(config4)
    nl = int(z["nlevels"])
    ops = [(z[f"rp{l}"], z[f"ci{l}"], z[f"v{l}"]) for l in range(nl)]
    ps = [None] + [(z[f"prp{l}"], z[f"pci{l}"], z[f"pv{l}"]) for l in range(1, nl)]
    lap = O.shifted_laplace(99, 99, 1, 2.0)  # natural order already local (kept by default): PMG_SELL_LOCALITY=2 is what reorders it
    for name, (rp, ci, v) in [("config4", ops[-1]), ("lap99x99", (lap.rowptr, lap.colidx, lap.vals))]:
        n = len(rp) - 1
        rng = np.random.default_rng(n)
        b, y0 = rng.standard_normal(n), rng.standard_normal(n)
        mc = MCSOR(rp, ci, v, COLORING_ITERATED).setup()
        out[f"meta/layout/{name}"] = mc.get_layout().astype(np.float64)
        for om, t in [(1.0, 1), (1.2, 3)]:
            mc.set_omega(om)
            mc.set_sweep_type(t)
            y = _dev(y0)
            mc.sample(_dev(b), y, 3, seed=0xD1CE, counter0=2)
            out[f"mcsor/{name}/om{om}/t{t}"] = _host(y)
        mc.destroy()
    n = len(ops[-1][0]) - 1
    rng = np.random.default_rng(4)
    b, y0 = rng.standard_normal(n), rng.standard_normal(n)
    for gz in (False, True):
        mg = MGMC.from_hierarchy(ops, ps)
        mg.set_smoother(True, 1.0, 3, 1)
        mg.setup()
        seen = []
        y = _dev(np.zeros(n) if gz else y0)
        mg.sample(_dev(b), y, 3, seed=0xF00D, counter0=0, guesszero=gz, callback=lambda it, yy: seen.append(_host(yy)))
        out[f"aijmg/config4/guesszero{int(gz)}"] = np.concatenate(seen)
        mg.destroy()


def main(argv):
    sys.path.insert(0, str(ROOT))
    import torch

    out = {}
    grid_runs(out)
    halo_run(out)
    mg_runs(out)
    aij_runs(out, argv[2])
    torch.cuda.synchronize()
    np.savez(argv[1], **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
