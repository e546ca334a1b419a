#!/usr/bin/env python3
"""Coloured block Gibbs (pmg_blockgibbs) against point Gibbs (pmg_mcsor_sample) on two operators, run on the GPU by hand
(never from bench.py):

  grid     the squared 5-point operator (L + shift I)^2 on 257 x 257 with vertex-star blocks (the 5-point stars, overlapping)
  lshape   the P1 matrix of tests/golden/lshape.msh refined 5 times (377 089 rows) with its greedy aggregates as blocks

Per operator one JSON line: ms per forward directional sweep of both samplers (device events around `--reps` noisy sweeps after
a warm-up), the byte model of a sweep and the fraction of 8 TB/s it gives at that time, and with --iact the integrated
autocorrelation time of one ball quantity of interest over 32 chains x 4000 steps (pmg_iact_chains, the reference's window rule)
with the time per effective sample = IACT x ms per sweep.  The chains are deterministic in their seeds, so the IACT part needs
one run; the timings are taken from fresh processes (tools/blockbench.py grid; tools/blockbench.py lshape; ...)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as sp

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

from parmgmc_amd import MCSOR, BlockGibbs, iact_chains
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
        for c in range(CHAINS):  # block Gibbs: chain after chain
            y.zero_()
            for s in range(a.steps):
                bg.sample(b, y, 1, seed=seeds[c], counter0=s)
                torch.dot(wd, y, out=X[s, c])
        tau, _, valid = iact_chains(X)
        out["block_iact"] = dict(median=float(np.median(tau)), min=float(tau.min()), max=float(tau.max()), valid=int(valid.sum()))
        for k in ("block", "point"):
            out[f"{k}_ms_per_effective_sample"] = out[f"{k}_iact"]["median"] * out[f"{k}_ms_per_sweep"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
