#!/usr/bin/env python3
"""Many chains per call on BASELINE config 4 (the unstructured line of bench.py): the sliced-ELL Gibbs sweep
(pmg_mcsor_sample_chains) and MGMC on the aggregation hierarchy (pmg_mgmc_sample_chains) for C chains, beside the
single-chain entry points.  Builds exactly what bench.py's unstructured_secondary builds: lshape.msh refined 5 times,
build_hierarchy(A, coarse_max=2000), PMG_COLORING_ITERATED, set_smoother(True, 1.0, 1, 1).

    python tools/chainbench.py [--chains 1 8 32 128] [--its 10] [--regions 5] [--lowrank K]

--stats: the chain statistics instead (pmg_chainstats_update, nqoi = 1 with weights): time per update on an (n, C) array,
algorithmic bytes 8 n C + 32 n + 8 n nqoi over that time, beside the read-2/write-1 triad (pmg_stream_triad on 4 n C / 3 doubles,
timed here in the same run) and beside the torch formulation of the same step (s = Y.sum(1); q = ((Y - (s/C)[:, None])**2).sum(1);
t = w @ Y; the merge on n-vectors); then MGMC chains with and without stats= (the added time per sample beside the update time).
--stats --iact: after these, per chain count one MGMC chains call of --iact-steps samples with stats= (timed), then on its trace
ChainStats.iact_device (pmg_chainstats_iact; wall time with the copy of the results) beside ChainStats.iact (the download and
pmg_iact per chain), their ratio, and the effective samples per second of sampling, sum_c steps / tau_c over the sampling time.

--lowrank K: posterior lines instead, with K ball observations on the mesh vertices (column j = indicator of the vertices
within --radius of centre j, divided by their count): the MATLRC sweep (mcgibbs, forward; pmg_mcsor_sample_chains on an
operator with pmg_mcsor_set_lowrank) and Woodbury + MGMC chains (WoodburySampler.run_chains on the per-chain right-hand-side
MGMC call), each beside its single-chain entry point (mcsor sample; the WoodburySampler.run loop); and MATLRC MGMC, the V-cycle on
the hierarchy that carries the update on every level (MGMC.set_lowrank; mg.sample beside mg.sample_chains), one cycle per sample
as the Woodbury line, with its ratio to that line.  --matlrc-only: only the MATLRC MGMC chains calls (for runs under rocprofv3).

--rb: the Rao-Blackwellised statistics instead (pmg_rbstats_update on the fine operator with b): time per update on an (n, C)
array, its algorithmic bytes 12 nnz + 8 n C + 48 n over that time, pmg_chainstats_update (no QOI) on the same Y in the same run,
the triad on the update's bytes and on those of one chains residual pass (12 nnz + 16 n C + 8 n); then MGMC chains plain, with
stats= and with rb=.

--cov: the covariance-error lines instead (pmg_chaincov_update; the config-4 mesh is not built): for n in {1024, 4096} x C in
{32, 1000}, time per update (median of `regions` event-timed groups of 20 updates), n (n + 1) C flops over that time against the
78.6 TFLOP/s f64 matrix peak of the vendor's data sheet, and at n = 1024 the host path on the same data: the device -> host copy of Y
plus pmg_estimate_covariance_errors per sample index (two indices minus one, so that its dense inverse is not counted); then MGMC
chains on the ex6 operator (32 x 32, kappa 1e-2, the hierarchy of the ex6 tests) at C = 1000 with and without cov=.

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
    ap.add_argument("--lowrank", type=int, default=0, help="K > 0: the posterior lines with K ball observations")
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--matlrc-only", action="store_true", help="with --lowrank: only the MATLRC MGMC chains calls (for runs under rocprofv3)")
    ap.add_argument("--stats", action="store_true", help="the chain-statistics lines (pmg_chainstats_update)")
    ap.add_argument("--iact", action="store_true", help="with --stats: the IACT of every chain on the device beside the host path, effective samples per second")
    ap.add_argument("--iact-steps", type=int, default=1000, help="with --iact: steps of the MGMC chains call whose trace is analysed")
    ap.add_argument("--rb", action="store_true", help="the Rao-Blackwellised statistics lines (pmg_rbstats_update beside pmg_chainstats_update on the same Y)")
    ap.add_argument("--cov", action="store_true", help="the covariance-error lines (pmg_chaincov_update)")
    ap.add_argument("--cov-updates-only", action="store_true", help="with --cov: only the update groups (for runs under rocprofv3)")
    args = ap.parse_args()
    if args.cov:
        return cov_lines(args)

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
    if args.stats:
        return stats_lines(args, n, mg, b)
    if args.rb:
        return rb_lines(args, A, mc, mg, b)
    if args.lowrank:
        return lowrank_lines(args, xy, A, mg, b, ops, ps)
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


def timed_all(fn, regions):
    """timed() that also returns the spread: (median, min, max) in ms"""
    import torch

    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def stats_lines(args, n, mg, b):
    import torch

    from parmgmc_amd import ChainStats
    from parmgmc_amd.capi import check, lib

    reps, nqoi = 20, 1
    gen = torch.Generator(device="cuda").manual_seed(1)
    w = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    for C in args.chains:
        Y = torch.randn((n, C), dtype=torch.float64, device="cuda", generator=gen)
        cs = ChainStats(n, C, [w], max_steps=reps * (args.regions + 1))

        def fused():
            for _ in range(reps):
                cs.update(Y)

        ms_f = timed(fused, args.regions) / reps
        alg = 8.0 * n * C + 32.0 * n + 8.0 * n * nqoi
        # the triad on the same number of bytes: 24 bytes per entry
        nt = int(alg / 24.0) & ~1
        a3, b3, c3 = (torch.zeros(nt, dtype=torch.float64, device="cuda") for _ in range(3))
        st = torch.cuda.current_stream().cuda_stream

        def triad():
            for _ in range(reps):
                check(lib.pmg_stream_triad(nt, a3.data_ptr(), b3.data_ptr(), c3.data_ptr(), st))

        ms_t = timed(triad, args.regions) / reps
        del a3, b3, c3
        # what a caller writes today: three passes over Y and the merge on n-vectors
        state = {"N": 0.0, "mean": torch.zeros(n, dtype=torch.float64, device="cuda"), "M2": torch.zeros(n, dtype=torch.float64, device="cuda")}

        def torch_step():
            for _ in range(reps):
                s = Y.sum(1)
                bm = s / C
                q = ((Y - bm[:, None]) ** 2).sum(1)
                t = w @ Y  # noqa: F841
                N1 = state["N"] + C
                d = bm - state["mean"]
                state["mean"] = state["mean"] + d * (C / N1)
                state["M2"] = state["M2"] + q + d * d * (state["N"] * C / N1)
                state["N"] = N1

        ms_p = timed(torch_step, args.regions) / reps
        rec = {"chains": C, "nqoi": nqoi, "update_us": ms_f * 1e3, "algorithmic_bytes": alg, "update_GBps": alg / ms_f / 1e6, "triad_us_same_bytes": ms_t * 1e3, "triad_GBps": 24.0 * nt / ms_t / 1e6,
               "update_over_triad_bandwidth": (alg / ms_f) / (24.0 * nt / ms_t), "torch_us": ms_p * 1e3, "torch_over_fused": ms_p / ms_f}
        print(json.dumps(rec), flush=True)
        del Y, cs, state
        torch.cuda.empty_cache()
    # MGMC chains with and without stats=
    its = args.its
    for C in args.chains:
        if C < 2:
            continue
        seeds = [0xCAFE + 7919 * c for c in range(C)]
        Y = torch.zeros((n, C), dtype=torch.float64, device="cuda")
        cs = ChainStats(n, C, [w], max_steps=its * (args.regions + 1))
        plain = timed_all(lambda: mg.sample_chains(b, Y, its, seeds), args.regions)
        with_stats = timed_all(lambda: mg.sample_chains(b, Y, its, seeds, stats=cs), args.regions)
        # a callback alone makes the sampler write the natural-order copy after every sample: the fair baseline of the difference
        print(json.dumps({"chains": C, "its": its, "mgmc_ms_per_sample": plain[0] / its, "mgmc_spread_ms_per_sample": [plain[1] / its, plain[2] / its],
                          "mgmc_stats_ms_per_sample": with_stats[0] / its, "mgmc_stats_spread_ms_per_sample": [with_stats[1] / its, with_stats[2] / its],
                          "added_us_per_sample": (with_stats[0] - plain[0]) / its * 1e3, "steps_recorded": cs.count()[0]}), flush=True)
        del Y, cs
        torch.cuda.empty_cache()
    if args.iact:
        iact_lines(args, n, mg, b, w)


def rb_lines(args, A, mc, mg, b):
    """pmg_rbstats_update on the fine operator: time per update (median of `regions` event-timed groups of 20 updates) beside
    pmg_chainstats_update on the same Y in the same run, the read-2/write-1 triad on the update's algorithmic bytes
    (12 nnz + 8 n C + 48 n) and on those of one chains residual pass (12 nnz + 16 n C + 8 n: the library has no entry point that
    runs that pass alone; the Gibbs sweep, which walks the same rows with the same gathers, is timed beside it), then the MGMC
    chains call with and without rb="""
    import torch

    from parmgmc_amd import ChainStats, RBStats
    from parmgmc_amd.capi import check, lib

    reps = 20
    n, nnz = A.shape[0], A.nnz
    gen = torch.Generator(device="cuda").manual_seed(1)
    st = torch.cuda.current_stream().cuda_stream

    def triad_us(nbytes):
        nt = int(nbytes / 24.0) & ~1
        a3, b3, c3 = (torch.zeros(nt, dtype=torch.float64, device="cuda") for _ in range(3))

        def triad():
            for _ in range(reps):
                check(lib.pmg_stream_triad(nt, a3.data_ptr(), b3.data_ptr(), c3.data_ptr(), st))

        return timed(triad, args.regions) / reps * 1e3

    for C in args.chains:
        Y = torch.randn((n, C), dtype=torch.float64, device="cuda", generator=gen)
        rb = RBStats(A, C, b=b)
        cs = ChainStats(n, C, [], max_steps=reps * (args.regions + 1))

        def rb_updates():
            for _ in range(reps):
                rb.update(Y)

        def cs_updates():
            for _ in range(reps):
                cs.update(Y)

        us_rb = timed(rb_updates, args.regions) / reps * 1e3
        us_cs = timed(cs_updates, args.regions) / reps * 1e3
        alg = rb.algorithmic_bytes()
        assert alg == 12.0 * nnz + 8.0 * n * C + 48.0 * n
        us_triad = triad_us(alg)
        us_resid = triad_us(12.0 * nnz + 16.0 * n * C + 8.0 * n)
        Ys = torch.zeros((n, C), dtype=torch.float64, device="cuda")
        us_sweep = timed(lambda: mc.sample_chains(b, Ys, args.its, [0xCAFE + 7919 * c for c in range(C)]), args.regions) / args.its * 1e3
        mean, var = rb.fields()
        rec = {"chains": C, "rb_update_us": us_rb, "algorithmic_bytes": alg, "rb_update_GBps": alg / us_rb / 1e3, "chainstats_update_us": us_cs, "triad_us_same_bytes": us_triad,
               "rb_over_triad_time": us_rb / us_triad, "triad_us_residual_bytes": us_resid, "rb_over_chainstats_plus_residual_triad": us_rb / (us_cs + us_resid), "gibbs_sweep_us": us_sweep,
               "finite": bool(torch.isfinite(mean).all().item() and torch.isfinite(var).all().item())}
        print(json.dumps(rec), flush=True)
        del Y, Ys, rb, cs
        torch.cuda.empty_cache()
    its = args.its
    for C in args.chains:
        seeds = [0xCAFE + 7919 * c for c in range(C)]
        Y = torch.zeros((n, C), dtype=torch.float64, device="cuda")
        rb = RBStats(A, C, b=b)
        cs = ChainStats(n, C, [], max_steps=its * (args.regions + 1))
        plain = timed_all(lambda: mg.sample_chains(b, Y, its, seeds), args.regions)
        with_stats = timed_all(lambda: mg.sample_chains(b, Y, its, seeds, stats=cs), args.regions)
        with_rb = timed_all(lambda: mg.sample_chains(b, Y, its, seeds, rb=rb), args.regions)
        print(json.dumps({"chains": C, "its": its, "mgmc_ms_per_sample": plain[0] / its, "mgmc_stats_ms_per_sample": with_stats[0] / its, "mgmc_rb_ms_per_sample": with_rb[0] / its,
                          "mgmc_rb_spread_ms_per_sample": [with_rb[1] / its, with_rb[2] / its], "rb_added_us_per_sample": (with_rb[0] - plain[0]) / its * 1e3,
                          "stats_added_us_per_sample": (with_stats[0] - plain[0]) / its * 1e3, "steps_recorded": rb.count()[0]}), flush=True)
        del Y, rb, cs
        torch.cuda.empty_cache()


def wall_ms(fn, regions):
    """median wall time in ms of fn(), which returns with its results on the host; one warm-up call first"""
    fn()
    ms = []
    for _ in range(regions):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms)[len(ms) // 2]


def iact_lines(args, n, mg, b, w):
    """one MGMC chains call of --iact-steps samples with stats= (timed), then on its trace: ChainStats.iact_device (wall time, the
    copy of the results included) beside ChainStats.iact (the download and pmg_iact per chain), and the effective samples per
    second of sampling, sum_c steps / tau_c over the sampling time"""
    import numpy as np
    import torch

    from parmgmc_amd import IACT_LAG_BLOCK, ChainStats

    steps = args.iact_steps
    for C in args.chains:
        if C < 2:
            continue
        seeds = [0xCAFE + 7919 * c for c in range(C)]
        Y = torch.zeros((n, C), dtype=torch.float64, device="cuda")
        cs = ChainStats(n, C, [w], max_steps=steps)
        mg.sample_chains(b, Y, 2, seeds)  # first-use workspace
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mg.sample_chains(b, Y, steps, seeds, stats=cs)
        torch.cuda.synchronize()
        sample_s = time.perf_counter() - t0
        dev_ms = wall_ms(lambda: cs.iact_device(0), args.regions)
        host_ms = wall_ms(lambda: cs.iact(0), args.regions)
        tau, window, valid = cs.iact_device(0)
        hosted = cs.iact(0)
        ok = np.isfinite(tau) & (tau > 0)
        ess = float((steps / tau[ok]).sum())
        print(json.dumps({"chains": C, "steps_recorded": cs.count()[0], "sampling_s": sample_s, "chain_samples_per_s": C * steps / sample_s,
                          "iact_device_ms": dev_ms, "iact_host_ms": host_ms, "host_over_device": host_ms / dev_ms,
                          "tau_min_median_max": [float(np.min(tau)), float(np.median(tau)), float(np.max(tau))], "window_max": int(window.max()), "chains_valid": int(valid.sum()),
                          "max_abs_tau_device_minus_host": float(np.max(np.abs(tau - np.array([t for t, _ in hosted])))),
                          "multiply_adds_model": float(steps) * float((window.astype(np.int64) // IACT_LAG_BLOCK + 1).sum()) * IACT_LAG_BLOCK,
                          "effective_samples": ess, "effective_samples_per_s": ess / sample_s}), flush=True)
        del Y, cs
        torch.cuda.empty_cache()


F64_MATRIX_PEAK = 78.6e12  # MI355X data sheet, FP64 matrix


def cov_lines(args):
    import numpy as np
    import torch

    import oracle as O
    from parmgmc_amd import MGMC, ChainCov, estimate_covariance_errors
    from parmgmc_amd.unstructured import build_hierarchy

    reps = 20
    gen = torch.Generator(device="cuda").manual_seed(1)
    for n in (1024, 4096):
        for C in (32, 1000):
            Y = torch.randn((n, C), dtype=torch.float64, device="cuda", generator=gen)
            cc = ChainCov.from_dense(np.eye(n), C, max_steps=reps * (args.regions + 1))

            def group():
                for _ in range(reps):
                    cc.update(Y)

            med, lo, hi = (t / reps for t in timed_all(group, args.regions))
            flops = float(n) * (n + 1) * C
            rec = {"n": n, "chains": C, "update_us": med * 1e3, "update_spread_us": [lo * 1e3, hi * 1e3], "flops": flops, "TFLOPs": flops / med / 1e9,
                   "fraction_of_f64_matrix_peak": flops / (med * 1e-3) / F64_MATRIX_PEAK, "steps_recorded": cc.count()}
            if n == 1024 and not args.cov_updates_only:
                A = O.ex6_matrix(32, 1e-2)
                t0 = time.perf_counter()
                Yh = Y.T.contiguous().cpu().numpy()
                copy_ms = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                estimate_covariance_errors(A.rowptr, A.colidx, A.vals, Yh, C)
                one = time.perf_counter() - t0
                t0 = time.perf_counter()
                estimate_covariance_errors(A.rowptr, A.colidx, A.vals, np.concatenate([Yh, Yh]), C)
                two = time.perf_counter() - t0
                host_ms = (two - one) * 1e3
                rec.update({"host_copy_ms": copy_ms, "host_ms_per_index": host_ms, "host_first_index_ms_with_inverse": one * 1e3, "host_over_device": (copy_ms + host_ms) / med})
            print(json.dumps(rec), flush=True)
            del Y, cc
            torch.cuda.empty_cache()
    if args.cov_updates_only:
        return
    A = O.ex6_matrix(32, 1e-2)
    ops, ps = build_hierarchy(A.scipy().tocsr(), coarse_max=100)
    mg = MGMC.from_hierarchy(ops, ps)
    mg.set_smoother(True, 1.0, 1, 1)
    mg.setup()
    n, C, its = A.n, 1000, args.its
    seeds = [0x5EED0000 + 7919 * c for c in range(C)]
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    Y = torch.zeros((n, C), dtype=torch.float64, device="cuda")
    cc = ChainCov.from_csr(A.rowptr, A.colidx, A.vals, C, max_steps=its * (args.regions + 1))
    plain = timed_all(lambda: mg.sample_chains(b, Y, its, seeds), args.regions)
    with_cov = timed_all(lambda: mg.sample_chains(b, Y, its, seeds, cov=cc), args.regions)
    print(json.dumps({"operator": "ex6 32 x 32", "chains": C, "its": its, "mgmc_ms_per_sample": plain[0] / its, "mgmc_spread_ms_per_sample": [plain[1] / its, plain[2] / its],
                      "mgmc_cov_ms_per_sample": with_cov[0] / its, "mgmc_cov_spread_ms_per_sample": [with_cov[1] / its, with_cov[2] / its],
                      "added_us_per_sample": (with_cov[0] - plain[0]) / its * 1e3, "steps_recorded": cc.count(), "last_error": float(cc.errors()[-1])}), flush=True)


def ball_centres(xy, k):
    """k mesh vertices as ball centres: the three quadrants' midpoints first, then vertices drawn with a fixed seed"""
    import numpy as np

    fixed = [(0.5, 0.5), (1.5, 0.5), (0.5, 1.5)]
    if k <= 3:
        return fixed[:k]
    rng = np.random.default_rng(0)
    return fixed + [tuple(xy[i]) for i in rng.choice(len(xy), size=k - 3, replace=False)]


def lowrank_lines(args, xy, A, mg, b, ops, ps):
    import numpy as np
    import torch

    from parmgmc_amd import COLORING_ITERATED, MCSOR, MGMC
    from parmgmc_amd.unstructured import ball_observations
    from parmgmc_amd.wrappers import WoodburySampler

    n, its, k = A.shape[0], args.its, args.lowrank
    B = ball_observations(xy, ball_centres(xy, k), args.radius)
    S = np.linspace(40.0, 80.0, k)
    # MGMC on the MATLRC hierarchy: the smoother and colouring of the prior hierarchy, the update on every level
    mgl = MGMC.from_hierarchy(ops, ps)
    mgl.set_coloring(COLORING_ITERATED)
    mgl.set_smoother(True, 1.0, 1, 1)
    mgl.set_lowrank(B, S)
    mgl.setup()
    if args.matlrc_only:
        for C in args.chains:
            seeds = [0xCAFE + 7919 * c for c in range(C)]
            Y = torch.zeros((n, C), dtype=torch.float64, device="cuda")
            ms = timed(lambda: mgl.sample_chains(b, Y, its, seeds), args.regions)
            print(json.dumps({"chains": C, "its": its, "lowrank": k, "matlrc_mgmc_ms_per_cycle": ms / its, "finite": bool(torch.isfinite(Y).all().item())}), flush=True)
        return
    mc = MCSOR(A.indptr, A.indices, A.data, COLORING_ITERATED).setup()
    mc.set_lowrank(B, S)
    # the Woodbury set-up's solver: ten symmetric Gauss-Seidel sweeps of the prior operator (its quality does not change the timing)
    gs = MCSOR(A.indptr, A.indices, A.data, COLORING_ITERATED).setup()
    gs.set_sweep_type(3)

    def solve(rhs, x):
        for _ in range(10):
            gs.apply(rhs, x)

    state = {"seed": 0xCAFE, "seeds": None}
    wb = WoodburySampler(B, S, solve, lambda w, y, ctr: mg.sample(w, y, 1, state["seed"], counter0=ctr),
                         sample_chains=lambda W, Y, ctr: mg.sample_chains(W, Y, 1, state["seeds"], counter0=ctr))
    print(json.dumps({"lowrank": k, "support_rows": int((np.abs(B).sum(1) > 0).sum()), "radius": args.radius}), flush=True)
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    ms1_sw = timed(lambda: mc.sample(b, y, its, seed=0xCAFE), args.regions)
    y.zero_()
    ms1_wb = timed(lambda: wb.run(b, y, its, 0xCAFE), args.regions)
    y.zero_()
    ms1_ml = timed(lambda: mgl.sample(b, y, its, seed=0xCAFE), args.regions)
    single = {"lowrank_sweep_samples_per_s": its * 1e3 / ms1_sw, "lowrank_sweep_ms": ms1_sw / its,
              "woodbury_mgmc_samples_per_s": its * 1e3 / ms1_wb, "woodbury_mgmc_ms": ms1_wb / its,
              "matlrc_mgmc_samples_per_s": its * 1e3 / ms1_ml, "matlrc_mgmc_ms": ms1_ml / its}
    print(json.dumps({"single_chain": single}), flush=True)
    for C in args.chains:
        seeds = [0xCAFE + 7919 * c for c in range(C)]
        state["seeds"] = seeds
        Y = torch.zeros((n, C), dtype=torch.float64, device="cuda")
        ms_sw = timed(lambda: mc.sample_chains(b, Y, its, seeds), args.regions)
        Y.zero_()
        ms_wb = timed(lambda: wb.run_chains(b, Y, its, seeds), args.regions)
        Y.zero_()
        ms_ml = timed(lambda: mgl.sample_chains(b, Y, its, seeds), args.regions)
        rec = {"chains": C, "its": its, "lowrank": k,
               "lowrank_sweep": {"chain_samples_per_s": C * its * 1e3 / ms_sw, "ms_per_call": ms_sw, "ms_per_sweep": ms_sw / its,
                                 "vs_single": (C * its * 1e3 / ms_sw) / single["lowrank_sweep_samples_per_s"]},
               "woodbury_mgmc": {"chain_samples_per_s": C * its * 1e3 / ms_wb, "ms_per_call": ms_wb, "ms_per_sample": ms_wb / its,
                                 "vs_single": (C * its * 1e3 / ms_wb) / single["woodbury_mgmc_samples_per_s"]},
               "matlrc_mgmc": {"chain_samples_per_s": C * its * 1e3 / ms_ml, "ms_per_call": ms_ml, "ms_per_cycle": ms_ml / its,
                               "roofline": mgl.algorithmic_bytes_chains(C)[0] / (ms_ml / its * 1e-3) / HBM_PEAK,
                               "vs_single": (C * its * 1e3 / ms_ml) / single["matlrc_mgmc_samples_per_s"], "time_over_woodbury_mgmc": ms_ml / ms_wb},
               "finite": bool(torch.isfinite(Y).all().item())}
        print(json.dumps(rec), flush=True)
        del Y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
