#!/usr/bin/env python3
"""Headline benchmark: Gaussian samples/sec of the red-black Gibbs sweep on a 512^3 DMDA (BASELINE.json).

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]

--steps K is the number of timed steps; "ms_per_step" in the JSON line is the time of one.  The timed steps run the chain
from x0 = 0 with noise counters 0..K-1 whatever the warm-up did, so the same arguments give the same result; with
--dump-outputs that result (the sample y after the last timed step) is written to DIR as .npy files, see dump_outputs().

N > 1: one rank per GPU.  Under torch.distributed.run (WORLD_SIZE set) this process IS a rank; started plainly it
spawns `python -m torch.distributed.run --nproc-per-node N bench.py ...` itself before touching a GPU and relays
rank 0's JSON line and the exit code.  A hang anywhere ends with "hang": true in the line and a non-zero exit code.

A "step" is ONE SAMPLE = one forward Gibbs sweep (= both colour passes, noise generated in-kernel) of the
sorgibbs/mcgibbs sampler on the 7-point operator of MatAssembleShiftedLaplaceFD (reference src/problems.c:14-75,
3-D analogue), kappa = 10, b = 1, x0 = 0, omega = 1 (reference examples/ex1.c:88,109), vectors resident in HBM
in the library's colour-partitioned layout.  N ranks split the SAME 512^3 grid into z-slabs ("strong" scaling)
and exchange one halo plane per colour per neighbour over xGMI (transport "ipc": peer stores + flag words;
fall-backs: RCCL ncclSend/ncclRecv from C, then torch.distributed P2P; PMG_DIST_TRANSPORT=ipc|rccl|torch forces one).

The JSON line also carries
  roofline     -- dominant kernel (grid_color_sweep_kernel, one colour pass): algorithmic bytes per launch
                  (24 B/unknown/sweep, SURVEY.md 8(d), x N/2 unknowns per launch = 12 N) / the average launch
                  duration measured here with HIP events on the launch stream, against the 8 TB/s HBM3E peak;
  cpu_baseline -- the CPU restatement of the reference's serial path (oracle/, lexicographic sweep + Box-Muller
                  noise, 1 core), timed on a bounded sample; reported, not the target.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: needed by RCCL and by the hipIpc halo transport

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)


def measured_traffic(n: int):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC summary of this same command
    (profiles/*_summary.json, written by tools/profile_bench.sh: separate --pmc FETCH_SIZE / WRITE_SIZE passes,
    gfx950 FETCH_SIZE x2 correction calibrated in-run).  None if no summary for this grid size is committed."""
    best = None
    for f in sorted((ROOT / "profiles").glob("*_summary.json")):
        try:
            d = json.loads(f.read_text())
        except Exception:
            continue
        if d.get("n") != n:
            continue
        for k in d["kernels"]:
            if k["kernel"].startswith("grid_color_sweep_kernel<true, true, false") and k.get("hbm_bytes_per_launch"):  # NOISY, OMEGA1, no halo
                best = (k["hbm_bytes_per_launch"], f.name)
    return best


def measured_cycle_traffic(key: str):
    """HBM bytes per SAMPLE of a secondary workload from the committed PMC summary (profiles/*_cycles_summary.json, written
    by tools/profile_cycles.sh: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE in separate passes over tools/cyclebench.py,
    read = 2 x FETCH_SIZE on gfx950, summed over every kernel launched between two samples).  None if absent."""
    best = None
    for f in sorted((ROOT / "profiles").glob("*_cycles_summary.json")):
        try:
            d = json.loads(f.read_text())
        except Exception:
            continue
        w = d.get("workloads", {}).get(key)
        if w and w.get("hbm_bytes_per_sample"):
            best = (w["hbm_bytes_per_sample"], f.name)
    return best


def cycle_roofline(alg_bytes: float, ms: float, key: str, n_gpus: int = 1, note: str = "") -> dict:
    """roofline dict of a secondary line: AS-BUILT algorithmic bytes of one sample (pmg_mgmc_get_algorithmic_bytes: every
    launch of the cycle counted with the operands it must read and write once -- DESIGN.md section 6 lists the per-kernel
    figures next to SURVEY 8(d)'s) / measured time per sample, against 8 TB/s per GPU"""
    ach = alg_bytes / (ms * 1e-3) / 1e9
    tr = measured_cycle_traffic(key) if n_gpus == 1 else None
    return {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS * n_gpus, "unit": "GB/s", "frac": ach / (HBM_PEAK_GBS * n_gpus), "traffic": tr[0] if tr else None, "traffic_source": tr[1] if tr else None, "algorithmic_bytes_per_sample": alg_bytes, "note": note or "as-built algorithmic bytes of one sample (sum over the kernels the cycle launches, each operand once) / time per sample"}


def usable_cores() -> int:
    """cores this process may actually use: scheduler affinity, capped by the cgroup CPU quota"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, q // per))
            break
        except Exception:  # noqa: BLE001
            continue
    # a GPU box shows all host cores but grants one GPU's share (16): without a visible limit, assume that share
    return min(n, int(os.environ.get("PMG_BENCH_CPU_THREADS", "16")))


def cpu_baseline(nsub: int = 512, nfull: int = 512, samples: int = 0) -> dict:
    """Serial reference path (one colour = lexicographic Gauss-Seidel, reference src/mc_sor.c:397-410,256-271;
    noise per reference src/parmgmc.c:99-110; RHS per src/pc_mcgibbs.c:119-128) on an nsub^3 grid, 1 core, built
    -O3 -march=native.  Default nsub = nfull = 512: the TRUE workload, 2 samples (about 18 GB of CSR + vectors and
    ~40 s with the assembly); a smaller nsub gives the sub-grid rate scaled by (nsub/nfull)^3."""
    import numpy as np

    import oracle as O

    if samples <= 0:
        samples = 2 if nsub >= 512 else 8
    L = O.lib(native=True)
    A = O.shifted_laplace(nsub, nsub, nsub, 10.0)
    n = A.n
    dp = O.diag_pointers(A)
    idg, sd = O.idiag(A, 1.0), O.sqrtdiag(A, 1.0, True)
    b, y, w = np.ones(n), np.zeros(n), np.zeros(n)
    L.orc_gibbs_sample_serial(n, A.rowptr, A.colidx, A.vals, dp, idg, sd, 1.0, b, y, w, 0xCAFE, 0)  # warm-up
    t0 = time.perf_counter()
    for s in range(samples):
        L.orc_gibbs_sample_serial(n, A.rowptr, A.colidx, A.vals, dp, idg, sd, 1.0, b, y, w, 0xCAFE, 1 + s)
    dt = time.perf_counter() - t0
    rate_sub = samples / dt
    out = {
        "value": rate_sub * (nsub / nfull) ** 3,
        "unit": "samples/s",
        "cores": 1,
        "kind": "port",
        "sample": (f"{samples} lexicographic Gibbs samples (CSR sweep + Box-Muller noise) on the full {nsub}^3 grid, {dt:.1f} s on 1 core" if nsub == nfull else f"{samples} lexicographic Gibbs samples (CSR sweep + Box-Muller noise) on a {nsub}^3 sub-grid = 1/{(nfull // nsub) ** 3} of the workload, {dt:.1f} s on 1 core; value = sub-grid rate x {(nsub / nfull) ** 3:g}"),
        "achieved_GBps_csr_model": (12 * len(A.vals) + 40 * n) * rate_sub / 1e9,
    }
    # the same sample on ALL host cores: red-black colouring, each colour one OpenMP loop over its rows (what the
    # reference does with one MPI rank per core and its parallel colouring); same bounded sub-grid
    try:
        cols = O.coloring_redblack(nsub, nsub, nsub)
        _nc, cptr, crows = O.color_lists(cols)
        L.orc_set_num_threads(usable_cores())  # the box's CPU share, not every core the host shows
        threads = L.orc_num_threads()
        y2 = np.zeros(n)
        L.orc_gibbs_sample_colored_parallel(n, 2, cptr, crows, A.rowptr, A.colidx, A.vals, dp, idg, sd, 1.0, b, y2, w, 0xCAFE, 0)
        reps = 2 * samples if nsub >= 512 else 4 * samples
        t0 = time.perf_counter()
        for s_ in range(reps):
            L.orc_gibbs_sample_colored_parallel(n, 2, cptr, crows, A.rowptr, A.colidx, A.vals, dp, idg, sd, 1.0, b, y2, w, 0xCAFE, 1 + s_)
        dt2 = time.perf_counter() - t0
        out["all_cores"] = {"value": reps / dt2 * (nsub / nfull) ** 3, "unit": "samples/s", "cores": threads, "kind": "port", "sample": f"{reps} red-black Gibbs samples (one OpenMP loop per colour) on the same {nsub}^3 grid, {dt2:.1f} s on {threads} threads", "achieved_GBps_csr_model": (12 * len(A.vals) + 40 * n) * reps / dt2 / 1e9}
    except Exception as e:  # noqa: BLE001
        out["all_cores"] = {"error": f"{type(e).__name__}: {e}"}
    return out


def mgmc_secondary(n: int = 257, levels: int = 5, its: int = 40) -> dict:
    """Secondary line (BASELINE config 1, "256^3 4-level V-cycle Gibbs, 1 MI355X", on the PETSc-coarsenable 257^3):
    samples/s of the Multigrid Monte Carlo chain (PCGAMGMC defaults: sorgibbs 1+1 sweeps per level, exact coarse
    sampler on 17^3).  Not the headline metric."""
    import torch

    from parmgmc_amd import MGMC

    t0 = time.perf_counter()
    mg = MGMC(n, n, n, 10.0, levels).setup()
    setup_s = time.perf_counter() - t0
    b = torch.ones(n ** 3, dtype=torch.float64, device="cuda")
    y = torch.zeros(n ** 3, dtype=torch.float64, device="cuda")
    ctr = mg.sample(b, y, 10, seed=0xCAFE)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    mg.sample(b, y, its, seed=0xCAFE, counter0=ctr)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / its
    alg, per = mg.algorithmic_bytes()
    return {"workload": f"{n}^3 DMDA, {levels}-level V-cycle MGMC sample (sorgibbs 1+1, cholsampler on {(n - 1) // 2 ** (levels - 1) + 1}^3)", "value": 1e3 / ms, "unit": "samples/s", "ms_per_sample": ms, "setup_s": setup_s, "roofline": cycle_roofline(alg, ms, f"mgmc_{n}_{levels}"), "algorithmic_bytes_per_unknown": alg / n ** 3, "algorithmic_bytes_per_level": [float(x) for x in per], "finite": bool(torch.isfinite(y).all().item())}


def stream_ceiling(n_doubles: int, reps: int = 20) -> dict:
    """The bandwidth a kernel with the colour sweep's access mix and NOTHING else reaches on this device (a measured
    device-copy / triad ceiling beside the vendor peak): pmg_stream_triad -- read two streams of n doubles, write one, 16 bytes
    per lane, a tile per workgroup -- over the sizes of one colour pass, HIP events on the launch stream."""
    import torch

    from parmgmc_amd.capi import check, lib

    n = n_doubles - (n_doubles & 1)
    a = torch.zeros(n, dtype=torch.float64, device="cuda")
    b = torch.ones(n, dtype=torch.float64, device="cuda")
    c = torch.empty(n, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(5):
        check(lib.pmg_stream_triad(n, a.data_ptr(), b.data_ptr(), c.data_ptr(), st))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        check(lib.pmg_stream_triad(n, a.data_ptr(), b.data_ptr(), c.data_ptr(), st))
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / reps * 1e3
    ok = bool((c[:: max(1, n // 4096)] == 0.5).all().item())
    return {"achieved": 24.0 * n / us / 1e3, "unit": "GB/s", "avg_launch_us": us, "launches": reps, "checked": ok, "kernel": "stream_triad_kernel: c = a + 0.5 b, 2 x 8 B read + 8 B written per entry, the sizes of one colour pass"}


def mgmc_lowrank_secondary(rank: int = 0, world: int = 1, transport=None, share: bool = False, n: int = 257, levels: int = 5, k: int = 3, its: int = 20) -> dict:
    """Secondary line (BASELINE config 5: "low-rank observation update on a 256^3 grid, dense coarse Cholesky on MFMA,
    4 GPUs"): the MGMC chain on A + B S B^T with k ball observations (reference src/obs.c:135-180,
    examples/ex4.c:150-168: radii 0.1 / 0.15 / 0.1, sigma^2 = 1e-4) on every level of the 257^3 hierarchy, coarse
    Cholesky of the explicit sum on 17^3, on `world` z-slabs (strong scaling; each rank holds its rows of B).
    Collective over all ranks.  Not the headline metric."""
    import numpy as np
    import torch
    import torch.distributed as dist

    from parmgmc_amd.dist import DistMGMC

    t0 = time.perf_counter()
    mg = DistMGMC(n, n, n, 10.0, levels, rank, world, transport=transport)
    k0, k1 = mg.plane_range
    from parmgmc_amd import make_observation_mats

    centres = [(0.25, 0.25, 0.25), (0.75, 0.75, 0.75), (0.25, 0.75, 0.5)] + [(0.5, 0.5, 0.1 + 0.8 * q / max(1, k - 4)) for q in range(max(0, k - 3))]
    radii = ([0.1, 0.15, 0.1] + [0.08] * max(0, k - 3))[:k]
    # MakeObservationMats on this rank's planes (library routine, src/obs.c:135-180 restated for the DMDA)
    B, S, f = make_observation_mats(n, n, n, np.asarray(centres[:k]).ravel(), radii, np.resize([1.0, -1.0], k), 1e-4, kz0=k0, nz_owned=k1 - k0)
    mg.set_lowrank(B, S)
    mg.setup()
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    b = torch.as_tensor(f, device="cuda")  # f = B S y_obs (src/obs.c:176-178)
    del B
    y = torch.zeros(mg.n_local, dtype=torch.float64, device="cuda")
    ctr = mg.sample(b, y, 3, seed=0xCAFE)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    mg.sample(b, y, its, seed=0xCAFE, counter0=ctr)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device="cpu" if share else "cuda")
    fin = torch.tensor([1.0 if bool(torch.isfinite(y).all().item()) else 0.0], dtype=torch.float64, device="cpu" if share else "cuda")
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(fin, op=dist.ReduceOp.MIN)
    ms = float(t.item()) / its * 1e3
    alg = torch.tensor([mg.algorithmic_bytes()[0]], dtype=torch.float64, device="cpu" if share else "cuda")
    if world > 1:
        dist.all_reduce(alg, op=dist.ReduceOp.SUM)
    res = {"roofline": cycle_roofline(float(alg.item()), ms, f"mgmc_lowrank_{n}_{levels}_k{k}", world, "as-built algorithmic bytes of one sample incl. the low-rank steps on their support rows (all ranks) / time per sample"), "workload": f"{n}^3 DMDA, {levels}-level V-cycle MGMC sample on A + B S B^T, k = {k} ball observations on every level (row-compact B, Bb), cholsampler of the explicit sum on {(n - 1) // 2 ** (levels - 1) + 1}^3, {world} z-slab(s)", "value": 1e3 / ms, "unit": "samples/s", "ms_per_sample": ms, "n_gpus": world, "transport": mg.transport, "setup_s": setup_s, "finite": bool(fin.item() == 1.0)}
    mg.destroy()
    return res


def unstructured_secondary(refine: int = 5, its: int = 50, larger: bool = True) -> dict:
    """Secondary line (BASELINE config 4: "unstructured GAMG hierarchy on data/lshape.msh, AIJ SpMV path, multicolour
    Gibbs, 1 GPU"): the reference's L-shape mesh (tests/golden/lshape.msh, a data fixture) refined `refine` times,
    P1 matrix kappa^2 M + K, aggregation hierarchy (parmgmc_amd/unstructured.py, host set-up), then on the device
    (a) the stand-alone multicolour Gibbs sampler on the fine MATAIJ matrix (sliced-ELL kernel, greedy colouring) and
    (b) the MGMC chain on the hierarchy.  Not the headline metric."""
    import torch

    from parmgmc_amd import MCSOR, MGMC
    from parmgmc_amd.unstructured import assemble_p1, build_hierarchy, read_gmsh41_triangles, refine_uniform

    t0 = time.perf_counter()
    xy, tris = read_gmsh41_triangles(ROOT / "tests" / "golden" / "lshape.msh")
    for _ in range(refine):
        xy, tris = refine_uniform(xy, tris)
    A = assemble_p1(xy, tris, 1.0)
    ops, ps = build_hierarchy(A, coarse_max=2000)
    host_s = time.perf_counter() - t0
    n, nnz = A.shape[0], A.nnz
    b = torch.ones(n, dtype=torch.float64, device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")

    def timed(fn, reps):
        fn(3, 0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(reps, 3)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    from parmgmc_amd import COLORING_ITERATED

    mc = MCSOR(A.indptr, A.indices, A.data, COLORING_ITERATED).setup()  # first-fit + one round of iterated greedy: 5 classes instead of 6 on these matrices
    ncol = mc.get_num_colors()
    ms_sweep = timed(lambda its_, c0: mc.sample(b, y, its_, seed=0xCAFE, counter0=c0, scaled=True), its)
    mg = MGMC.from_hierarchy(ops, ps)
    mg.set_coloring(COLORING_ITERATED)
    mg.set_smoother(True, 1.0, 1, 1)
    mg.setup()
    y.zero_()
    ms_mg = timed(lambda its_, c0: mg.sample(b, y, its_, seed=0xCAFE, counter0=c0), its)
    alg_mg = mg.algorithmic_bytes()[0]
    sell_note = "12 nnz + 40 N bytes per sweep (SURVEY 8(d): 8 B value + 4 B column per stored entry; rowptr, row index, idiag, b, y read, y write per row) / time per sweep"
    out = {"workload": f"lshape.msh refined {refine}x: P1 kappa^2 M + K, {n} rows, {nnz} nonzeros; aggregation hierarchy {[len(o[0]) - 1 for o in ops]}", "gibbs_sweep": {"value": 1e3 / ms_sweep, "unit": "samples/s", "ms_per_sample": ms_sweep, "colors": ncol, "coloring": "first-fit + one round of iterated greedy (PMG_COLORING_ITERATED)", "roofline": cycle_roofline(12 * nnz + 40 * n, ms_sweep, f"sell_sweep_{n}", 1, sell_note)}, "mgmc": {"value": 1e3 / ms_mg, "unit": "samples/s", "ms_per_sample": ms_mg, "levels": len(ops), "roofline": cycle_roofline(alg_mg, ms_mg, f"mgmc_aij_{n}")}, "host_setup_s": host_s, "finite": bool(torch.isfinite(y).all().item())}
    if larger:  # the same sweep one refinement further, where it is no longer bound by the latency of its dependent launches
        del mc, mg
        xy, tris = refine_uniform(xy, tris)
        A2 = assemble_p1(xy, tris, 1.0)
        b2 = torch.ones(A2.shape[0], dtype=torch.float64, device="cuda")
        y2 = torch.zeros(A2.shape[0], dtype=torch.float64, device="cuda")
        mc2 = MCSOR(A2.indptr, A2.indices, A2.data, COLORING_ITERATED).setup()
        ms2 = timed(lambda its_, c0: mc2.sample(b2, y2, its_, seed=0xCAFE, counter0=c0, scaled=True), its)
        out["gibbs_sweep_refined_once_more"] = {"rows": A2.shape[0], "nonzeros": A2.nnz, "ms_per_sample": ms2, "colors": mc2.get_num_colors(), "roofline": cycle_roofline(12 * A2.nnz + 40 * A2.shape[0], ms2, f"sell_sweep_{A2.shape[0]}", 1, sell_note)}
    return out


def mgmc_dist_secondary(rank: int, world: int, transport, share: bool, n: int = 513, levels: int = 6, its: int = 10) -> dict:
    """Secondary line (BASELINE config 3 flavour, "512^3 DMDA V-cycle on 8 MI355X", on the PETSc-coarsenable 513^3 with
    6 levels so that the exact coarse sampler works on 17^3): samples/s of the MGMC chain on `world` z-slabs -- the
    SAME 513^3 grid for every N (strong scaling).  Collective over all ranks.  Not the headline metric."""
    import torch
    import torch.distributed as dist

    from parmgmc_amd.dist import DistMGMC

    t0 = time.perf_counter()
    mg = DistMGMC(n, n, n, 10.0, levels, rank, world, transport=transport)
    mg.setup()
    setup_s = time.perf_counter() - t0
    b = torch.ones(mg.n_local, dtype=torch.float64, device="cuda")
    y = torch.zeros(mg.n_local, dtype=torch.float64, device="cuda")
    ctr = mg.sample(b, y, 2, seed=0xCAFE)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t1 = time.perf_counter()
    mg.sample(b, y, its, seed=0xCAFE, counter0=ctr)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t1
    t = torch.tensor([dt], dtype=torch.float64, device="cpu" if share else "cuda")
    fin = torch.tensor([1.0 if bool(torch.isfinite(y).all().item()) else 0.0], dtype=torch.float64, device="cpu" if share else "cuda")
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(fin, op=dist.ReduceOp.MIN)
    ms = float(t.item()) / its * 1e3
    alg = torch.tensor([mg.algorithmic_bytes()[0]], dtype=torch.float64, device="cpu" if share else "cuda")
    if world > 1:
        dist.all_reduce(alg, op=dist.ReduceOp.SUM)  # every rank's share (replicated levels count once per rank: they run on every rank)
    res = {"workload": f"{n}^3 DMDA, {levels}-level V-cycle MGMC sample (sorgibbs 1+1, cholsampler on {(n - 1) // 2 ** (levels - 1) + 1}^3), {world} z-slab(s), strong scaling", "value": 1e3 / ms, "unit": "samples/s", "ms_per_sample": ms, "n_gpus": world, "transport": mg.transport, "setup_s": setup_s, "roofline": cycle_roofline(float(alg.item()), ms, f"mgmc_{n}_{levels}", world), "algorithmic_bytes_per_unknown": float(alg.item()) / n ** 3, "finite": bool(fin.item() == 1.0)}
    mg.destroy()
    return res


def unstructured_dist_secondary(rank: int, world: int, transport, share: bool, refine: int = 5, its: int = 20) -> dict:
    """Secondary line (BASELINE config 4's matrix on N GPUs): the MGMC chain on the aggregation hierarchy of the refined
    lshape.msh P1 matrix, every level above the coarsest distributed by ROW BLOCKS (parmgmc_amd.dist.DistAIJMGMC: the
    reference's PCGAMGMC on a MATMPIAIJ), the same matrix for every N (strong scaling).  Collective.  Not the headline."""
    import torch
    import torch.distributed as dist

    from parmgmc_amd.dist import DistAIJMGMC
    from parmgmc_amd.unstructured import assemble_p1, build_hierarchy, read_gmsh41_triangles, refine_uniform

    t0 = time.perf_counter()
    xy, tris = read_gmsh41_triangles(ROOT / "tests" / "golden" / "lshape.msh")
    for _ in range(refine):
        xy, tris = refine_uniform(xy, tris)
    ops, ps = build_hierarchy(assemble_p1(xy, tris, 1.0), coarse_max=2000)
    from parmgmc_amd import COLORING_ITERATED

    mg = DistAIJMGMC(ops, ps, rank, world, transport=transport, coloring=COLORING_ITERATED)  # as the one-device line: 5 classes instead of 6, one ghost update fewer per sweep
    mg.set_smoother(True, 1.0, 1, 1)
    mg.setup()
    setup_s = time.perf_counter() - t0
    b = torch.ones(mg.n_owned, dtype=torch.float64, device="cuda")
    y = torch.zeros(mg.n_owned, dtype=torch.float64, device="cuda")
    ctr = mg.sample(b, y, 3, seed=0xCAFE)
    torch.cuda.synchronize()
    dist.barrier()
    t1 = time.perf_counter()
    mg.sample(b, y, its, seed=0xCAFE, counter0=ctr)
    torch.cuda.synchronize()
    dist.barrier()
    dt = time.perf_counter() - t1
    dev = "cpu" if share else "cuda"
    t = torch.tensor([dt], dtype=torch.float64, device=dev)
    fin = torch.tensor([1.0 if bool(torch.isfinite(y).all().item()) else 0.0], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.all_reduce(fin, op=dist.ReduceOp.MIN)
    ms = float(t.item()) / its * 1e3
    alg = torch.tensor([mg.algorithmic_bytes()[0]], dtype=torch.float64, device=dev)
    dist.all_reduce(alg, op=dist.ReduceOp.SUM)
    res = {"roofline": cycle_roofline(float(alg.item()), ms, "", world), "workload": f"lshape.msh refined {refine}x: {len(ops[-1][0]) - 1} rows, aggregation hierarchy {[len(o[0]) - 1 for o in ops]}, row blocks over {world} ranks, strong scaling", "value": 1e3 / ms, "unit": "samples/s", "ms_per_sample": ms, "n_gpus": world, "transport": mg.transport, "setup_s": setup_s, "finite": bool(fin.item() == 1.0)}
    mg.destroy()
    return res


DUMP_FULL_MAX = 1 << 22  # unknowns: up to 32 MB of f64 the whole sample is written
DUMP_SAMPLE = 1 << 21  # above that: this many entries at fixed seeded positions (16 MB of values + 16 MB of indices)


def dump_outputs(dirpath: str, g, y, n: int, rank: int, world: int) -> dict:
    """--dump-outputs: what the timed steps computed, as the caller of the sampler receives it -- the sample y after the
    last timed step, in the natural (i fastest) order of the whole n^3 grid, f64.  Up to DUMP_FULL_MAX unknowns:
    y.npy holds every entry.  Above: y_sample.npy holds DUMP_SAMPLE entries at positions drawn once from a fixed seed
    (the same for every run with the same --grid-n) and y_sample_index.npy those positions (exact in f64).  Collective
    over all ranks (each contributes its z-slab); rank 0 writes.  Returns {name: shape} of the files written."""
    import numpy as np
    import torch
    import torch.distributed as dist

    from parmgmc_amd.slab import slab_cuts

    total = n ** 3
    off = slab_cuts(n, world)[rank] * n * n  # the first global index of this rank's slab
    nat = g.from_cvec(y)
    if total <= DUMP_FULL_MAX:
        idx = None
        mine = nat.cpu().numpy()
    else:
        idx = np.sort(np.random.default_rng(0x5EED).choice(total, size=DUMP_SAMPLE, replace=False))
        sel = idx[(idx >= off) & (idx < off + g.n)] - off
        mine = nat[torch.as_tensor(sel, device=nat.device)].cpu().numpy()
    del nat
    parts = [None] * world
    if world > 1:
        dist.all_gather_object(parts, mine)
    else:
        parts[0] = mine
    if rank != 0:
        return {}
    vals = np.ascontiguousarray(np.concatenate(parts), dtype=np.float64)  # slabs are contiguous in z: rank order = index order
    assert vals.size == (total if idx is None else DUMP_SAMPLE), vals.size
    out = Path(dirpath)
    out.mkdir(parents=True, exist_ok=True)
    arrays = {"y": vals} if idx is None else {"y_sample": vals, "y_sample_index": idx.astype(np.float64)}
    for name, a in arrays.items():
        np.save(out / f"{name}.npy", a)
    return {name: list(a.shape) for name, a in arrays.items()}


def spawn_ranks(n: int, argv: list) -> int:
    """`python bench.py --gpus N` with N > 1 and no torchrun environment: start N fresh ranks (one per GPU) as a child
    `python -m torch.distributed.run` BEFORE this process imports torch or touches a GPU, pass their output through
    (rank 0 prints the JSON line) and return the child's exit code.  A child that outlives the limit is killed with its
    whole process group and reported as a hang (non-zero)."""
    import signal
    import socket
    import subprocess

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve()), *argv]
    limit = float(os.environ.get("PMG_BENCH_SPAWN_TIMEOUT", "1500"))
    child = subprocess.Popen(cmd, start_new_session=True)
    try:
        return child.wait(timeout=limit)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(child.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        child.wait()
        print(json.dumps({"metric": METRIC, "value": None, "unit": "samples/s", "n_gpus": n, "hang": True, "error": f"ranks still running after {limit:.0f} s: killed"}), flush=True)
        return 3
    except KeyboardInterrupt:
        os.killpg(child.pid, signal.SIGKILL)
        raise


METRIC = "Gaussian samples/sec on 512^3 3D DMDA (7-pt Laplacian precision, red-black Gibbs sweep = 1 sorgibbs sample)"


class Watchdog:
    """A collective or a device wait that never returns must not look like success: when the deadline passes, rank 0
    prints what it has with "hang": true and EVERY rank leaves with exit code 3 (torchrun then reports failure)."""

    def __init__(self, rank: int, world: int, steps: int, warmup: int):
        self.rank, self.world, self.steps, self.warmup = rank, world, steps, warmup
        self.out, self.stage, self.timer, self.printed = None, "start", None, threading.Event()

    def arm(self, seconds: float, stage: str):
        self.cancel()
        self.stage = stage
        self.timer = threading.Timer(seconds, self._fire)
        self.timer.daemon = True
        self.timer.start()

    def cancel(self):
        if self.timer is not None:
            self.timer.cancel()
            self.timer = None

    def _fire(self):
        if self.rank == 0 and not self.printed.is_set():
            self.printed.set()
            line = dict(self.out) if self.out else {"metric": METRIC, "value": None, "unit": "samples/s", "n_gpus": self.world, "steps": self.steps, "warmup": self.warmup}
            line["hang"] = True
            line["hang_stage"] = self.stage
            print(json.dumps(line), flush=True)
        os._exit(3)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20, help="untimed steps (a clock-settle phase of its own follows them, see settle())")
    ap.add_argument("--grid-n", dest="n", type=int, default=512, help="grid points per direction (default: the BASELINE 512^3)")
    ap.add_argument("--omega", type=float, default=1.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-n", type=int, default=512, help="grid of the CPU baseline (512 = the true workload; smaller: sub-grid rate scaled)")
    ap.add_argument("--no-mgmc", action="store_true", help="skip the secondary V-cycle lines")
    ap.add_argument("--no-settle", action="store_true", help="skip the clock-settle phase")
    ap.add_argument("--mgmc-n", type=int, default=513, help="grid of the distributed V-cycle line (2^k + 1)")
    ap.add_argument("--mgmc-levels", type=int, default=6)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write the sample they computed as DIR/<name>.npy (see dump_outputs())")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product has no CPU path)")
    # rehearsal on a one-GPU box: PMG_BENCH_SHARE_DEVICE=1 puts every rank on cuda:0 and bootstraps over gloo (RCCL
    # cannot run two ranks on one device); the sweep kernels, the schedule and the "ipc" halo transport are the real ones
    share = os.environ.get("PMG_BENCH_SHARE_DEVICE") == "1"
    if share:
        local = 0
    dog = Watchdog(rank, world, args.steps, args.warmup)
    dog.arm(float(os.environ.get("PMG_BENCH_HEADLINE_TIMEOUT", "420")), "headline")
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    cdev = "cpu" if (share or world == 1) else "cuda"  # where the small agreement tensors live

    from parmgmc_amd.dist import DistGridSampler

    n = args.n
    seed = 0xCAFE

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def agree(ok: bool) -> bool:
        """True iff `ok` on every rank.  Every rank reaches every collective of measure() whatever failed locally:
        local errors are carried in flags, never raised between two collectives"""
        flag = torch.tensor([1 if ok else 0], device=cdev)
        if world > 1:
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return int(flag.item()) == 1

    def settle(smp, b, y, ctr):
        """Clock-settle phase, independent of --warmup: after idle the first launches run fast, the next few dozen up to
        40 % slower, then the clocks settle.  Untimed groups of 5 sweeps (10 colour launches) with an event between
        groups run until three consecutive group means agree within 2 %; capped at 3 rounds of 32 groups (~0.3 s at
        512^3 on one GPU).  All ranks take the decision together (the sample loop is collective over the halos)."""
        groups, per, launches, hist = 32, 5, 0, []
        for _round in range(3):
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(groups + 1)]
            evs[0].record()
            for g_ in range(groups):
                ctr = smp.sample_cvec(b, y, per, seed, ctr)
                evs[g_ + 1].record()
            torch.cuda.synchronize()
            ms = [evs[i].elapsed_time(evs[i + 1]) / per for i in range(groups)]
            hist += ms
            launches += 2 * per * groups
            last = ms[-3:]
            ok = max(last) <= 1.02 * min(last)
            if agree(ok):
                break
        hs = sorted(hist[-groups:])
        return ctr, {"settle_launches": launches, "settle_ms_per_step_first": hist[0], "settle_ms_per_step_worst": max(hist), "settle_ms_per_step_last": hist[-1], "settle_ms_per_step_median_last_round": hs[len(hs) // 2]}

    def measure(transport):
        """warm-up + settle + timed region on one halo transport; returns everything the JSON line needs.  Never raises
        between collectives: a local failure is recorded and agreed on at the end"""
        err = None
        smp = DistGridSampler(n, n, n, 10.0, rank, world, omega=args.omega, transport=transport)  # agrees on its transport itself
        g = smp.grid
        nat_b = torch.ones(g.n, dtype=torch.float64, device="cuda")
        b = g.to_cvec(nat_b)
        del nat_b
        y = g.new_cvec()  # x0 = 0
        ctr, st = 0, {}
        try:
            ctr = smp.sample_cvec(b, y, args.warmup, seed, 0)
            if not args.no_settle:
                ctr, st = settle(smp, b, y, ctr)
        except Exception as e:  # noqa: BLE001
            err = f"warm-up: {type(e).__name__}: {e}"
        if not agree(err is None):  # nobody enters the timed region unless everybody can
            return dict(smp=smp, err=err or "warm-up failed on another rank", ok=False)
        # the timed region starts the chain afresh (x0 = 0, noise counters from 0): what it computes then depends on the
        # arguments alone, not on how many sweeps the adaptive settle phase took
        y.zero_()
        ctr = timed_from = 0
        barrier()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        ev0.record()
        try:
            ctr = smp.sample_cvec(b, y, args.steps, seed, ctr)
        except Exception as e:  # noqa: BLE001
            err = f"timed region: {type(e).__name__}: {e}"
        ev1.record()
        barrier()
        dt = time.perf_counter() - t0
        dev_ms = ev0.elapsed_time(ev1)  # HIP events on the launch stream (torch's current stream is the one passed to the C-ABI)
        try:
            smp.check()  # a device-side wait for a halo flag that gave up shows here
        except Exception as e:  # noqa: BLE001
            err = err or f"{type(e).__name__}: {e}"
        tmax = torch.tensor([dt], dtype=torch.float64, device=cdev)
        ranks = None
        if world > 1:
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            # a self-describing record: every rank says where it ran, whether its device reaches its
            # z-neighbours' devices as peers, how long ITS timed region took and how often its face wavefronts had to poll
            # for a halo flag; gathered to rank 0.  Under torchrun the neighbours' device indices are their local ranks
            # (every process sees all devices of the node); with PMG_BENCH_SHARE_DEVICE all ranks sit on device 0.
            try:
                lo_dev = -1 if rank == 0 else (0 if share else local - 1)
                hi_dev = -1 if rank == world - 1 else (0 if share else local + 1)
                me = smp.describe(lo_dev, hi_dev)
            except Exception as e:  # noqa: BLE001
                me = {"rank": rank, "error": f"{type(e).__name__}: {e}"}
            me.update({"local_rank": local, "timed_region_s": dt, "device_ms": dev_ms, "host": os.uname().nodename, "hip_visible_devices": os.environ.get("HIP_VISIBLE_DEVICES") or os.environ.get("ROCR_VISIBLE_DEVICES")})
            ranks = [None] * world
            dist.all_gather_object(ranks, me)
        finite = bool(torch.isfinite(y).all().item())
        # multi-GPU only, outside the timed region: rank 0 repeats the whole chain on ITS device alone and compares its
        # slab bit for bit (the noise depends on global indices only, so the distributed chain must reproduce it exactly)
        halo_check = None
        if err is None and world > 1 and rank == 0 and os.environ.get("PMG_BENCH_NO_HALO_CHECK") != "1":
            from parmgmc_amd import GridMCSOR

            one = GridMCSOR(n, n, n, 10.0)
            one.set_omega(args.omega)
            ob = one.to_cvec(torch.ones(one.n, dtype=torch.float64, device="cuda"))
            oy = one.new_cvec()
            one.sample_cvec(ob, oy, ctr, seed, 0, True)
            mine = g.from_cvec(y)
            ref = one.from_cvec(oy)[: mine.numel()]
            halo_check = "bit-identical to the single-device chain (rank 0's slab)" if torch.equal(mine, ref) else f"MISMATCH vs the single-device chain: max abs diff {float((mine - ref).abs().max()):.3e}"
            del one, ob, oy, mine, ref
            torch.cuda.empty_cache()
        good = err is None and (halo_check is None or halo_check.startswith("bit-identical"))
        ok = agree(good)
        return dict(smp=smp, g=g, y=y, b=b, dt=float(tmax.item()), dev_ms=dev_ms, finite=finite, halo_check=halo_check, settle=st, err=err, ok=ok, chain_len=ctr, timed_from=timed_from, ranks=ranks)

    # N > 1: the transports in order of preference; one that fails at run time (lost flag, wrong halo data) is dropped
    # and the next one measured -- decided by rank 0's bit-for-bit check, agreed by all ranks
    forced = os.environ.get("PMG_DIST_TRANSPORT") or ("ipc" if (share and world > 1) else None)
    order = [forced] if (forced or world == 1) else ["ipc", "rccl", "torch"]
    res, tried = None, []
    for tr in order:
        res = measure(tr)
        tried.append({"transport": tr, "actual": res["smp"].transport, "ok": res["ok"], "error": res["err"], "halo_check": res.get("halo_check")})
        if res["ok"]:
            break
        if rank == 0:
            print(f"[bench] halo transport {tr!r} rejected: {res['err'] or res.get('halo_check') or 'failed on another rank'}", file=sys.stderr, flush=True)
        res["smp"].destroy()  # collective, orderly: the next transport allocates and exports fresh blocks
        res = None
        torch.cuda.empty_cache()
    if res is None:
        if rank == 0:
            print(json.dumps({"metric": METRIC, "value": None, "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "error": "no halo transport produced a valid chain", "transports_tried": tried}), flush=True)
        sys.exit(4)
    smp, g, y, b, dt, dev_ms, finite, halo_check = (res[k] for k in ("smp", "g", "y", "b", "dt", "dev_ms", "finite", "halo_check"))
    used_transport = smp.transport
    dumped = dump_outputs(args.dump_outputs, g, y, n, rank, world) if args.dump_outputs else None

    if rank == 0:
        N_total = n * n * n
        N_local = g.n
        launches = 2 * args.steps  # one launch per colour
        t_launch = dev_ms * 1e-3 / launches
        alg_bytes_per_launch = (24 if args.omega == 1.0 else 32) * N_local / 2
        achieved = alg_bytes_per_launch / t_launch / 1e9
        traffic = measured_traffic(n) if (world == 1 and args.omega == 1.0) else None
        out = {
            "metric": METRIC,
            "value": args.steps / dt,
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": f"{n}^3 DMDA, 7-point shifted Laplacian (kappa=10, h2=1/(n-1)^2), b=1, x0=0, omega={args.omega:g}, forward red-black Gibbs sweep with in-kernel Philox4x32-10 + Box-Muller noise", "unknowns": N_total, "decomposition": f"{world} z-slab(s)", "halo": "none" if world == 1 else {"ipc": "1 plane/colour/neighbour, stored by the face blocks of the sweep kernel straight into the neighbour's receive block over xGMI (hipIpc peer memory), announced by a flag word the neighbour's face wavefronts wait for inside the same launch", "rccl": "1 plane/colour/neighbour over RCCL ncclSend/ncclRecv", "torch": "1 plane/colour/neighbour over torch.distributed P2P (RCCL)"}[smp.transport], "transport": smp.transport},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic[0] if traffic else None, "traffic_source": traffic[1] if traffic else None, "kernel": "grid_color_sweep_kernel", "algorithmic_bytes_per_launch": alg_bytes_per_launch, "avg_launch_us": t_launch * 1e6, "note": "24 B/unknown/sweep (read y, write y, read b once; SURVEY 8(d)) x N/2 unknowns per colour launch; duration = HIP-event time of the timed region / launches"},
            "finite": finite,
            "clock_settle": res["settle"],
        }
        if world == 1 and os.environ.get("PMG_BENCH_NO_CEILING") != "1":
            try:  # measured ceiling of the access mix, beside the vendor peak `frac` is taken against
                sc = stream_ceiling(N_local // 2)
                sc["sweep_over_ceiling"] = achieved / sc["achieved"]
                out["roofline"]["stream_ceiling"] = sc
            except Exception as e:  # never allowed to cost the headline line
                out["roofline"]["stream_ceiling"] = {"error": f"{type(e).__name__}: {e}"}
        if dumped:
            out["dump_outputs"] = {"dir": str(Path(args.dump_outputs).resolve()), "arrays": dumped}
        if halo_check is not None:
            out["halo_check"] = halo_check
        if res.get("ranks"):
            rk = res["ranks"]
            ts = sorted(r.get("timed_region_s", float("nan")) for r in rk)
            out["ranks_seen"] = {"torch_world_size": dist.get_world_size(), "records": len(rk), "rccl_comm_count": max((r.get("rccl_comm_count", 0) for r in rk), default=0), "distinct_devices": len({(r.get("host"), r.get("pci_bus_id")) for r in rk})}
            out["timed_region_s"] = {"min": ts[0], "median": ts[len(ts) // 2], "max": ts[-1]}
            out["halo_wait_polls_total"] = sum(int(r.get("halo_wait_polls", 0)) for r in rk)
            out["ranks"] = rk
        if len(tried) > 1:
            out["transports_tried"] = tried
        dog.out = out
    else:
        out = None
    # ---- secondary lines: never allowed to cost the headline line -------------------------------------------------
    def emit():
        if rank == 0 and not dog.printed.is_set():
            dog.printed.set()
            print(json.dumps(out), flush=True)

    if not args.no_mgmc and os.environ.get("PMG_BENCH_NO_MGMC") != "1":
        smp.destroy()  # collective: unmap peers, barrier, free -- the secondary lines build their own transports
        del b, y, smp, g, res
        torch.cuda.empty_cache()
        dog.arm(float(os.environ.get("PMG_BENCH_SECONDARY_TIMEOUT", "300")), "secondary lines")  # a hang here: headline printed with "hang": true, exit code 3
        try:
            if world == 1:
                out["secondary_mgmc"] = mgmc_secondary()
                try:
                    out["secondary_unstructured"] = unstructured_secondary()
                except Exception as e:  # noqa: BLE001
                    out["secondary_unstructured"] = {"error": f"{type(e).__name__}: {e}"}
            tr2 = used_transport if used_transport in ("ipc", "rccl") else None
            try:
                sec = mgmc_lowrank_secondary(rank, world, tr2, share)
            except Exception as e:  # noqa: BLE001
                sec = {"error": f"{type(e).__name__}: {e}"}
            if rank == 0:
                out["secondary_mgmc_lowrank"] = sec
            sec = mgmc_dist_secondary(rank, world, used_transport if used_transport in ("ipc", "rccl") else None, share, args.mgmc_n, args.mgmc_levels)
            if rank == 0:
                out["secondary_mgmc_dist"] = sec
            if world > 1 and tr2:
                sec = unstructured_dist_secondary(rank, world, tr2, share)
                if rank == 0:
                    out["secondary_unstructured_dist"] = sec
        except Exception as e:  # noqa: BLE001
            if rank == 0:
                out.setdefault("secondary_mgmc_dist", {"error": f"{type(e).__name__}: {e}"})
                if "secondary_mgmc_dist" in out and "error" not in out["secondary_mgmc_dist"]:
                    out["secondary_unstructured_dist"] = {"error": f"{type(e).__name__}: {e}"}
    dog.cancel()
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args.cpu_n, n)
    emit()
    if world > 1:
        dog.arm(60.0, "destroy_process_group")
        dist.destroy_process_group()
        dog.cancel()


if __name__ == "__main__":
    main()
