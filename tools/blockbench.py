#!/usr/bin/env python3
"""Coloured block Gibbs (pmg_blockgibbs) against point Gibbs (pmg_mcsor_sample) on two operators, run on the GPU by hand
(never from bench.py):

  grid     the squared 5-point operator (L + shift I)^2 on 257 x 257 with vertex-star blocks (the 5-point stars, overlapping)
  lshape   the P1 matrix of tests/golden/lshape.msh refined 5 times (377 089 rows) with its greedy aggregates as blocks

Per operator one JSON line: ms per forward directional sweep of both samplers (device events around `--reps` noisy sweeps after
a warm-up), the byte model of a sweep and the fraction of 8 TB/s it gives at that time, and with --iact the integrated
autocorrelation time of one ball quantity of interest over 32 chains x 4000 steps (pmg_iact_chains, the reference's window rule)
with the time per effective sample = IACT x ms per sweep.  --chains C1,C2,... (default 1,8,32,128) adds, per C, the block sampler
advancing C chains per launch (pmg_blockgibbs_sample_chains) under the same protocol: ms per noisy forward sweep of all chains,
chain-sweeps per second, the chains byte model and its fraction of 8 TB/s, next to the single-chain line (DESIGN.md section
12.1); --chains "" leaves it out.  The chains are deterministic in their seeds, so the IACT part needs one run (both samplers
advance all 32 chains per launch); the timings are taken from fresh processes (tools/blockbench.py grid; tools/blockbench.py
lshape; ...)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

from parmgmc_amd import MCSOR, BlockGibbs, ChainStats, iact_chains
from parmgmc_amd.unstructured import assemble_p1, ball_observations, greedy_aggregation, read_gmsh41_triangles, refine_uniform

PEAK = 8e12  # bytes per second
CHAINS, STEPS = 32, 4000


def grid_case(n, shift):
    T = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
    A1 = (sp.kron(sp.identity(n), T) + sp.kron(T, sp.identity(n)) + shift * sp.identity(n * n)).tocsr()
    A1.sort_indices()
    A = (A1 @ A1).tocsr()
    A.sort_indices()
    blocks = (A1.indptr.astype(np.int32), A1.indices.astype(np.int32))  # block v = the stored columns of row v of the 5-point operator
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="xy"), -1).reshape(-1, 2) / (n - 1.0)
    w = (np.linalg.norm(ij - 0.5, axis=1) <= 0.1).astype(np.float64)
    return A, blocks, w / w.sum()


def lshape_case(refine, kappa):
    xy, tris = read_gmsh41_triangles(ROOT / "tests" / "golden" / "lshape.msh")
    for _ in range(refine):
        xy, tris = refine_uniform(xy, tris)
    A = assemble_p1(xy, tris, kappa)
    P = greedy_aggregation(A).tocsc()  # column a = the rows of aggregate a
    centre = xy[np.argmin(np.linalg.norm(xy - xy.mean(axis=0), axis=1))]
    w = np.asarray(ball_observations(xy, centre[None, :], 0.1 * np.ptp(xy[:, 0])))[:, 0]
    return A, (P.indptr.astype(np.int32), P.indices.astype(np.int32)), w


def timed(sample, reps):
    sample(20, 0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    sample(reps, 20)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["grid", "lshape"])
    ap.add_argument("--n", type=int, default=257)
    ap.add_argument("--shift", type=float, default=0.5)
    ap.add_argument("--refine", type=int, default=5)
    ap.add_argument("--kappa", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--iact", action="store_true")
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--chains", default="1,8,32,128", help="chain counts of the block sampler's chains form, comma separated")
    a = ap.parse_args()
    A, blocks, w = grid_case(a.n, a.shift) if a.case == "grid" else lshape_case(a.refine, a.kappa)
    n, nnz = A.shape[0], A.nnz
    bg = BlockGibbs(A.indptr, A.indices, A.data, blocks).setup()
    mc = MCSOR(A.indptr, A.indices, A.data).setup()
    sizes = np.diff(blocks[0])
    out = dict(case=a.case, rows=n, nnz=nnz, blocks=len(sizes), slots=int(sizes.sum()), block_rows_min_max=[int(sizes.min()), int(sizes.max())], block_colours=bg.get_num_colors(), point_colours=mc.get_num_colors())
    b = torch.ones(n, dtype=torch.float64, device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    out["block_ms_per_sweep"] = timed(lambda its, c0: bg.sample(b, y, its, seed=1, counter0=c0), a.reps)
    y.zero_()
    out["point_ms_per_sweep"] = timed(lambda its, c0: mc.sample(b, y, its, seed=1, counter0=c0, scaled=True), a.reps)
    out["block_bytes"], out["point_bytes"] = bg.algorithmic_bytes(), 12.0 * nnz + 40.0 * n
    for k in ("block", "point"):
        out[f"{k}_fraction_of_8TBs"] = out[f"{k}_bytes"] / (out[f"{k}_ms_per_sweep"] * 1e-3) / PEAK
    out["block_chain_sweeps_per_s"] = 1e3 / out["block_ms_per_sweep"]
    out["block_chains"] = []
    for nc in [int(v) for v in a.chains.split(",") if v]:
        Yc = torch.zeros(n, nc, dtype=torch.float64, device="cuda")
        seeds = list(range(1, 1 + nc))
        ms = timed(lambda its, c0: bg.sample_chains(b, Yc, its, seeds, counter0=c0), a.reps)
        nbytes = bg.algorithmic_bytes_chains(nc)
        out["block_chains"].append(dict(chains=nc, ms_per_sweep=ms, chain_sweeps_per_s=nc * 1e3 / ms, bytes=nbytes, fraction_of_8TBs=nbytes / (ms * 1e-3) / PEAK,
                                        speedup_over_single_chain=nc * out["block_ms_per_sweep"] / ms))
        del Yc
    if a.iact:
        wd = torch.as_tensor(w, device="cuda")
        X = torch.empty(a.steps, CHAINS, dtype=torch.float64, device="cuda")
        Y = torch.zeros(n, CHAINS, dtype=torch.float64, device="cuda")
        seeds = list(range(100, 100 + CHAINS))
        b.zero_()  # the chains start in the mean of their target: no transient in the series
        y.zero_()
        for s in range(a.steps):  # point Gibbs: all chains per launch
            mc.sample_chains(b, Y, 1, seeds, counter0=s, scaled=True)
            torch.matmul(wd, Y, out=X[s])
        tau, _, valid = iact_chains(X)
        out["point_iact"] = dict(median=float(np.median(tau)), min=float(tau.min()), max=float(tau.max()), valid=int(valid.sum()))
        # block Gibbs: all chains per launch, one call for all steps; column c is the chain bg.sample(seed=seeds[c]) gives, and the
        # library's own callback records w . Y[:, c] of every step on the device (no Python in the loop)
        cs = ChainStats(n, CHAINS, qois=[w], max_steps=a.steps)
        Y.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bg.sample_chains(b, Y, a.steps, seeds, counter0=0, stats=cs)
        torch.cuda.synchronize()
        out["block_iact_wall_s"] = time.perf_counter() - t0
        tau, _, valid = cs.iact_device(0)
        out["block_iact"] = dict(median=float(np.median(tau)), min=float(tau.min()), max=float(tau.max()), valid=int(valid.sum()))
        for k in ("block", "point"):
            out[f"{k}_ms_per_effective_sample"] = out[f"{k}_iact"]["median"] * out[f"{k}_ms_per_sweep"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
