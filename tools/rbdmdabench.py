#!/usr/bin/env python3
"""The matrix-free Rao-Blackwellised statistics handle on a DMDA grid (pmg_rbstats_create_dmda) beside the CSR handle on the
assembled operator (development tool).

    tools/rbdmdabench.py --n 129 257 513 --repeat 3 --out profiles/rbstats_dmda_measurements.json
        runs every size in `repeat` fresh child processes, the sizes alternating, and writes the median and the range over the
        processes of every figure.  The parent process does not touch the GPU.
    tools/rbdmdabench.py --child --n 257 [--mgmc] [--no-csr]
        one process, one JSON line: at n^3, C = 1, b = ones, kappa = 10
          update_us            pmg_rbstats_update per call, DMDA and CSR handle in the same process (median of `regions` event-timed
                               groups of `reps` calls, after a warm-up group)
          triad_us             pmg_stream_triad on the DMDA update's algorithmic bytes (48 n), in the same run
          chainstats_us        pmg_chainstats_update on the same Y
          setup_s, device_bytes  creation + first update (host clock, synchronised) and the drop of free device memory over it
          same_bits            the fields of the two handles after the timed updates are equal bit for bit
        --mgmc: ms per sample of the 5-level MGMC with rb= the DMDA handle, rb= the CSR handle and neither, and of the cycle with
        k = 3 ball observations (pmg_mgmc_set_lowrank) with and without rb= a DMDA handle that carries the same (B, S).
        --kernel-only: 5 updates of the DMDA handle and nothing else (for a counters run of the kernel alone).
A CSR handle at 513^3 needs about 11 GB of host matrix and is not built (--no-csr is implied there)."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
KAPPA, LEVELS = 10.0, 5


def timed_all(fn, regions):
    """(median, min, max) in ms of fn() over `regions` event-timed calls after one warm-up call"""
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


def timed_alternating(fns, regions):
    """{name: (median, min, max) in ms}: every region times each function of `fns` once, in turn, after one warm-up call of each"""
    import torch

    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(regions):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: (sorted(v)[len(v) // 2], min(v), max(v)) for name, v in ms.items()}


def free_bytes():
    import torch

    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def observations(n, k=3):
    """the ball observations of tools/record_cycle_bytes.py"""
    import numpy as np

    from parmgmc_amd import make_observation_mats

    centres = [(0.25, 0.25, 0.25), (0.75, 0.75, 0.75), (0.25, 0.75, 0.5)]
    B, S, _ = make_observation_mats(n, n, n, np.asarray(centres[:k]).ravel(), [0.1, 0.15, 0.1][:k], np.resize([1.0, -1.0], k), 1e-4)
    return B, S


def child(args):
    import torch

    import oracle as O
    from parmgmc_amd import MGMC, ChainStats, RBStats
    from parmgmc_amd.capi import check, lib

    n1 = args.n[0]
    n = n1**3
    reps, regions = args.reps, args.regions
    b = torch.ones(n, dtype=torch.float64, device="cuda")
    Y = torch.randn(n, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    st = torch.cuda.current_stream().cuda_stream

    def make(kind):
        f0, t0 = free_bytes(), time.perf_counter()
        rb = RBStats.dmda(n1, n1, n1, KAPPA, b=b) if kind == "dmda" else RBStats(O.shifted_laplace(n1, n1, n1, KAPPA), 1, b=b)
        rb.update(Y)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rb.reset()
        return rb, t1 - t0, f0 - free_bytes()

    def updates(h):
        def run():
            for _ in range(reps):
                h.update(Y)

        return run

    if args.kernel_only:
        rb, _, _ = make("dmda")
        for _ in range(5):
            rb.update(Y)
        torch.cuda.synchronize()
        print(json.dumps({"n": n1, "kernel_only_updates": 6}))
        return
    rec = {"n": n1, "rows": n, "reps": reps, "regions": regions}
    dm, rec["dmda_setup_s"], rec["dmda_device_bytes"] = make("dmda")
    rec["dmda_algorithmic_bytes"] = alg = dm.algorithmic_bytes()
    assert alg == 48.0 * n
    csr = None
    if not args.no_csr and n1 < 513:
        csr, rec["csr_setup_s"], rec["csr_device_bytes"] = make("csr")
        rec["csr_algorithmic_bytes"] = csr.algorithmic_bytes()
    # the handles alternate region by region, so that a drift of the clocks hits both alike
    kinds = {"dmda": updates(dm)} if csr is None else {"dmda": updates(dm), "csr": updates(csr)}
    for kind, (med, lo, hi) in timed_alternating(kinds, regions).items():
        rec[f"{kind}_update_us"] = med / reps * 1e3
        rec[f"{kind}_update_us_range"] = [lo / reps * 1e3, hi / reps * 1e3]
    rec["dmda_update_GBps"] = alg / rec["dmda_update_us"] / 1e3
    nt = int(alg / 24.0) & ~1
    a3, b3, c3 = (torch.zeros(nt, dtype=torch.float64, device="cuda") for _ in range(3))

    def triad():
        for _ in range(reps):
            check(lib.pmg_stream_triad(nt, a3.data_ptr(), b3.data_ptr(), c3.data_ptr(), st))

    t = timed_all(triad, regions)
    rec["triad_us"], rec["triad_us_range"] = t[0] / reps * 1e3, [t[1] / reps * 1e3, t[2] / reps * 1e3]
    rec["triad_over_dmda_time"] = rec["triad_us"] / rec["dmda_update_us"]
    del a3, b3, c3
    cs = ChainStats(n, 1, [], max_steps=reps * (regions + 1))
    t = timed_all(updates(cs), regions)
    rec["chainstats_us"] = t[0] / reps * 1e3
    del cs
    if csr is not None:
        rec["csr_over_dmda_time"] = rec["csr_update_us"] / rec["dmda_update_us"]
        for h in (dm, csr):
            h.reset()
            h.update(Y)
            h.update(b)
        rec["same_bits"] = all(bool(torch.equal(x, y)) for x, y in zip(dm.fields(), csr.fields()))
    if args.mgmc:
        its = args.its
        y = torch.zeros(n, dtype=torch.float64, device="cuda")
        mg = MGMC(n1, n1, n1, KAPPA, LEVELS).setup()
        def sampler(m, h):
            return lambda: m.sample(b, y, its, seed=1, rb=h)

        with_rb = {"none": sampler(mg, None), "dmda": sampler(mg, dm)}
        if csr is not None:
            with_rb["csr"] = sampler(mg, csr)
        for name, t in timed_alternating(with_rb, regions).items():
            rec[f"mgmc_rb_{name}_ms_per_sample"], rec[f"mgmc_rb_{name}_ms_range"] = t[0] / its, [t[1] / its, t[2] / its]
        mg.destroy()
        del csr
        torch.cuda.empty_cache()
        B, S = observations(n1)
        mg = MGMC(n1, n1, n1, KAPPA, LEVELS)
        mg.set_lowrank(B, S)
        mg.setup()
        f0, t0 = free_bytes(), time.perf_counter()
        dm.set_lowrank(B, S)
        dm.update(Y)
        torch.cuda.synchronize()
        rec["dmda_k3_setup_s"], rec["dmda_k3_device_bytes_added"] = time.perf_counter() - t0, f0 - free_bytes()
        rec["dmda_k3_algorithmic_bytes"] = dm.algorithmic_bytes()
        t = timed_all(updates(dm), regions)
        rec["dmda_k3_update_us"] = t[0] / reps * 1e3
        for name, t in timed_alternating({"none": sampler(mg, None), "dmda": sampler(mg, dm)}, regions).items():
            rec[f"mgmc_k3_rb_{name}_ms_per_sample"], rec[f"mgmc_k3_rb_{name}_ms_range"] = t[0] / its, [t[1] / its, t[2] / its]
        rec["finite"] = bool(torch.isfinite(y).all().item())
    print(json.dumps(rec), flush=True)


def parent(args):
    runs = {n: [] for n in args.n}
    for r in range(args.repeat):
        for n in args.n:  # the sizes alternate; every measurement is a fresh process
            cmd = [sys.executable, __file__, "--child", "--n", str(n), "--reps", str(args.reps), "--regions", str(args.regions), "--its", str(args.its)]
            if args.mgmc and n == args.mgmc_n:
                cmd.append("--mgmc")
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
            if out.returncode != 0:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                raise SystemExit(f"the child for n = {n} ended with status {out.returncode}: no further GPU process is started")
            rec = json.loads(out.stdout.strip().splitlines()[-1])
            print(json.dumps(rec), flush=True)
            runs[n].append(rec)
    summary = {"protocol": f"{args.repeat} fresh processes per size, the sizes alternating; per process the median of {args.regions} device-event-timed groups of {args.reps} calls after a warm-up group; here the median and [min, max] over the processes", "kappa": KAPPA, "sizes": {}}
    for n, recs in runs.items():
        s = {}
        for key in recs[0]:
            vals = [r[key] for r in recs if key in r]
            if all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in vals):
                v = sorted(vals)
                s[key] = {"median": v[len(v) // 2], "range": [v[0], v[-1]]}
            elif all(isinstance(v, bool) for v in vals):
                s[key] = all(vals)
        s["processes"] = recs
        summary["sizes"][str(n)] = s
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(summary, indent=1) + "\n")
    print(json.dumps({k: {m: v["median"] for m, v in s.items() if isinstance(v, dict)} for k, s in summary["sizes"].items()}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[129, 257])
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--no-csr", action="store_true")
    ap.add_argument("--mgmc", action="store_true")
    ap.add_argument("--mgmc-n", type=int, default=257)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--its", type=int, default=10)
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child or args.kernel_only:
        child(args)
    else:
        parent(args)


if __name__ == "__main__":
    main()
