#!/usr/bin/env python3
"""Many chains per call on BASELINE config 4 (the unstructured line of bench.py): the sliced-ELL Gibbs sweep
(pmg_mcsor_sample_chains) and MGMC on the aggregation hierarchy (pmg_mgmc_sample_chains) for C chains, beside the
single-chain entry points.  Builds exactly what bench.py's unstructured_secondary builds: lshape.msh refined 5 times,
build_hierarchy(A, coarse_max=2000), PMG_COLORING_ITERATED, set_smoother(True, 1.0, 1, 1).

    python tools/chainbench.py [--chains 1 8 32 128] [--its 10] [--regions 5]

Time per call = median over `regions` event-timed regions of one call of `its` samples each.  Aggregate rate = C * its /
time.  Roofline fraction = algorithmic bytes (sweep: 12 nnz + 24 N + 16 N C; MGMC: pmg_mgmc_get_algorithmic_bytes_chains)
/ time, against 8 TB/s.  One JSON line per chain count."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_PEAK = 8.0e12


def timed(fn, regions):
    import torch

    fn()  # warm-up (first-use workspace, key upload)
    torch.cuda.synchronize()
    ms = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--its", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--refine", type=int, default=5)
    ap.add_argument("--sweep-only", action="store_true", help="only the chains sweep (for counter runs under rocprofv3)")
    args = ap.parse_args()

    import torch

    from parmgmc_amd import COLORING_ITERATED, MCSOR, MGMC
    from parmgmc_amd.unstructured import assemble_p1, build_hierarchy, read_gmsh41_triangles, refine_uniform

    t0 = time.perf_counter()
    xy, tris = read_gmsh41_triangles(ROOT / "tests" / "golden" / "lshape.msh")
    for _ in range(args.refine):
        xy, tris = refine_uniform(xy, tris)
    A = assemble_p1(xy, tris, 1.0)
    ops, ps = build_hierarchy(A, coarse_max=2000)
    n, nnz = A.shape[0], A.nnz
    mc = MCSOR(A.indptr, A.indices, A.data, COLORING_ITERATED).setup()
    mg = None
    if not args.sweep_only:
        mg = MGMC.from_hierarchy(ops, ps)
        mg.set_coloring(COLORING_ITERATED)
        mg.set_smoother(True, 1.0, 1, 1)
        mg.setup()
    print(json.dumps({"workload": f"lshape.msh refined {args.refine}x, {n} rows, {nnz} nonzeros, hierarchy {[len(o[0]) - 1 for o in ops]}", "colors": mc.get_num_colors(), "host_setup_s": time.perf_counter() - t0}), flush=True)

    b = torch.ones(n, dtype=torch.float64, device="cuda")
    its = args.its
    if args.sweep_only:
        for C in args.chains:
            Y = torch.zeros((n, C), dtype=torch.float64, device="cuda")
            ms = timed(lambda: mc.sample_chains(b, Y, its, [0xCAFE + 7919 * c for c in range(C)]), args.regions)
            print(json.dumps({"chains": C, "sweep_ms_per_call": ms, "algorithmic_bytes_per_sweep": 12.0 * nnz + 24.0 * n + 16.0 * n * C, "finite": bool(torch.isfinite(Y).all().item())}), flush=True)
        return
    # single-chain entry points
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    ms1_sw = timed(lambda: mc.sample(b, y, its, seed=0xCAFE), args.regions)
    y.zero_()
    ms1_mg = timed(lambda: mg.sample(b, y, its, seed=0xCAFE), args.regions)
    alg1_mg = mg.algorithmic_bytes()[0]
    single = {"sweep_samples_per_s": its * 1e3 / ms1_sw, "sweep_ms": ms1_sw / its, "sweep_roofline": (12 * nnz + 40 * n) / (ms1_sw / its * 1e-3) / HBM_PEAK,
              "mgmc_samples_per_s": its * 1e3 / ms1_mg, "mgmc_ms": ms1_mg / its, "mgmc_roofline": alg1_mg / (ms1_mg / its * 1e-3) / HBM_PEAK}
    print(json.dumps({"single_chain": single}), flush=True)
    for C in args.chains:
        seeds = [0xCAFE + 7919 * c for c in range(C)]
        Y = torch.zeros((n, C), dtype=torch.float64, device="cuda")
        ms_sw = timed(lambda: mc.sample_chains(b, Y, its, seeds), args.regions)
        Y.zero_()
        ms_mg = timed(lambda: mg.sample_chains(b, Y, its, seeds), args.regions)
        alg_sw = 12.0 * nnz + 24.0 * n + 16.0 * n * C
        alg_mg = mg.algorithmic_bytes_chains(C)[0]
        rec = {"chains": C, "its": its,
               "sweep": {"chain_samples_per_s": C * its * 1e3 / ms_sw, "ms_per_call": ms_sw, "ms_per_sweep": ms_sw / its, "roofline": alg_sw / (ms_sw / its * 1e-3) / HBM_PEAK,
                         "vs_single": (C * its * 1e3 / ms_sw) / single["sweep_samples_per_s"]},
               "mgmc": {"chain_samples_per_s": C * its * 1e3 / ms_mg, "ms_per_call": ms_mg, "ms_per_cycle": ms_mg / its, "roofline": alg_mg / (ms_mg / its * 1e-3) / HBM_PEAK,
                        "vs_single": (C * its * 1e3 / ms_mg) / single["mgmc_samples_per_s"]},
               "finite": bool(torch.isfinite(Y).all().item())}
        print(json.dumps(rec), flush=True)
        del Y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
