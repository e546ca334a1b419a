"""Child process of test_gpu_lrc_ranks.py: the single-level samplers (MCSOR on CSR, GridMCSOR) with a low-rank update of
every rank and storage form of CASES, run once each in a fresh process (under rocprofv3 --kernel-trace when the parent has
it, so that the parent can tell which kernels each case ran) and written raw to an .npz.

Every case starts with set_lowrank, whose set-up ends with exactly two launches of lrc_gemm_small_kernel (Bb = C Sb, one
per sweep direction), and ends with one launch of torch's spin_kernel (torch.cuda._sleep) as a marker; the parent cuts the
trace at both.

    python lrc_rank_workloads.py <out.npz>
"""
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
if __name__ == "__main__":
    sys.path[:0] = [str(ROOT), str(HERE)]

import oracle as O  # noqa: E402
from test_lrc import ball_matrix  # noqa: E402

RANKS = [1, 8, 9, 33, 64]
# path -> (grid, observation kind, PMG_* environment at set_lowrank, omega)
#   small: ns <= 1024 support rows (one block of the row-compact kernels); rows: several blocks; dense: support > ld / 4
#   *_fused: PMG_LRC_FUSED=1 -- the noise term in one kernel; with ns <= 1024 B^T y and its update in one workgroup
PATHS = {
    "small": ((17, 17, 17), "points", {}, 1.0),
    "small_fused": ((17, 17, 17), "points", {"PMG_LRC_FUSED": "1"}, 1.15),
    "rows": ((33, 33, 33), "balls", {}, 1.0),
    "rows_fused": ((33, 33, 33), "balls", {"PMG_LRC_FUSED": "1"}, 1.15),
    "dense": ((17, 17, 9), "wide", {}, 1.0),
}
SAMPLERS = ["csr", "grid"]
CASES = [(s, k, p) for s in SAMPLERS for k in RANKS for p in PATHS]
SWEEPS = [(1, True), (2, False), (3, True)]  # (sweep type, scaled)


def sweep_settings(omega):
    """the sweeps of a case; the unscaled (sorgibbs) noise needs omega = 1"""
    return [(sweep, scaled or omega != 1.0) for sweep, scaled in SWEEPS]
SEED, CTR0, ITS, KAPPA = 9, 4, 3, 2.0
ZERO_COLUMN = 17  # the k = 64 sets have an empty ball here: a zero column of B


def observations(grid, kind, k, seed):
    """B (n x k) and S (k) of one case"""
    nx, ny, nz = grid
    n = nx * ny * nz
    rng = np.random.default_rng(seed)
    if kind == "points":  # one grid point per ball: the support of B and Bb = 7 rows a column at most
        pts = rng.choice([(i, j, l) for i in range(1, nx - 1) for j in range(1, ny - 1) for l in range(1, nz - 1)], size=k, replace=False)
        centres = [(i / (nx - 1), j / (ny - 1), l / (nz - 1)) for i, j, l in pts]
        radii = [0.3 / (nx - 1)] * k
    elif kind == "balls":  # balls of ~1500 / k points each: 1024 < joint support < ld / 4
        r = (1500.0 / k / (4.19 * (nx - 1) ** 3)) ** (1 / 3)
        centres = [tuple(rng.uniform(0.2, 0.8, 3)) for _ in range(k)]
        radii = list(rng.uniform(0.9 * r, 1.1 * r, k))
    else:  # wide: every column on a third of the rows
        B = np.zeros((n, k))
        for c in range(k):
            idx = rng.choice(n, size=n // 3, replace=False)
            B[idx, c] = rng.uniform(0.5, 1.5, len(idx)) / len(idx)
        return B, rng.uniform(20.0, 90.0, k)
    if k == 64:
        radii[ZERO_COLUMN] = 0.0
    B = ball_matrix(grid, centres, radii)
    if k == 64:
        assert not B[:, ZERO_COLUMN].any()
    assert np.count_nonzero(np.abs(B).sum(0)) == k - (k == 64)
    return B, rng.uniform(20.0, 90.0, k)


def case_inputs(sampler, k, path):
    grid, kind, env, omega = PATHS[path]
    B, S = observations(grid, kind, k, 1000 * k + len(path))
    n = int(np.prod(grid))
    rng = np.random.default_rng(k)
    return dict(grid=grid, B=B, S=S, b=rng.standard_normal(n), y0=rng.standard_normal(n), env=env, omega=omega)


def case_key(sampler, k, path):
    return f"{sampler}/k{k}/{path}"


def main(out_path):
    import torch

    from parmgmc_amd import MCSOR, GridMCSOR

    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")
    host = lambda t: t.detach().cpu().numpy().copy()
    out = {}
    for sampler, k, path in CASES:
        c = case_inputs(sampler, k, path)
        for key in [e for e in os.environ if e.startswith("PMG_LRC_")]:
            del os.environ[key]
        os.environ.update(c["env"])
        key = case_key(sampler, k, path)
        if sampler == "grid":
            s = GridMCSOR(*c["grid"], KAPPA)
        else:
            A = O.shifted_laplace(*c["grid"], KAPPA)
            s = MCSOR(A.rowptr, A.colidx, A.vals).setup()
            out[f"{key}/colors"] = s.get_coloring()
        out[f"{key}/ld"] = np.array(s.cvec_len if sampler == "grid" else s.layout_len())
        s.set_omega(c["omega"])
        s.set_lowrank(c["B"], c["S"])
        for sweep, scaled in sweep_settings(c["omega"]):
            s.set_sweep_type(sweep)
            bd, yd = dev(c["b"]), dev(c["y0"])
            s.apply(bd, yd)
            out[f"{key}/apply{sweep}"] = host(yd)
            yd = dev(c["y0"])
            s.sample(bd, yd, ITS, seed=SEED, counter0=CTR0, scaled=scaled)
            out[f"{key}/sample{sweep}"] = host(yd)
            out[f"{key}/b{sweep}"] = host(bd)
        torch.cuda._sleep(100)  # the end of this case's launches
        torch.cuda.synchronize()
        s.destroy()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
