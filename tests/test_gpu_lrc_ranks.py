"""The low-rank (MATLRC) update A + B S B^T over its whole rank range 1 <= k <= 64 (pmg_lrc.c, kernels_lrc.hip).

Ranks 1, 8, 9, 33 and 64: one column (half a Box-Muller pair), both sides of the k <= 8 switch of the row-compact update,
an odd rank, more than 32 columns, and every LDS slot of the 64-column kernels.  For every rank each storage form and
kernel path the host picks is driven and pinned:

  - single-level samplers (MCSOR on CSR, GridMCSOR; lrc_rank_workloads.py in a child process under rocprofv3's kernel
    trace): deterministic apply against O.lrc_mcsor_apply (1e-12) and 3-sample chains against O.lrc_gibbs_samples (1e-11)
    for forward, backward and symmetric sweeps, in the dense form, the row-compact form with one and with several blocks of
    support rows, and both with PMG_LRC_FUSED=1 (the noise term drawn in the kernel; one workgroup for B^T y and its update).
    The trace must show the kernels of that path, and launch sizes that match the support the oracle predicts.
  - MGMC whole chains against LrcMgmcOracle (test_lrc.py, 1e-10): grid level, class-stencil levels, sliced-ELL levels,
    Cholesky and Gibbs coarse samplers, both correction forms.  The storage form of every level is asserted through
    level_lowrank_factors.  A negative control requires the device to miss a k = 64 oracle with the last column's S or eta
    changed by far more than the tolerance.
  - MGMC at 65^3, where several blocks of support rows exist on the finest levels: each low-rank step once against numpy
    on the factors the device holds.
  - Whole chains of the folded default against its switched-off forms and the fused form, bit for bit, at k = 9 and 64.
  - The exact coarse sampler of A + B S B^T at k = 64; re-setting the update on a live sampler; rank -1 and 65 rejected.
"""
import csv
import math
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle as O
import lrc_rank_workloads as W
from test_lrc import ETA_TAG, M64, LrcMgmcOracle, ball_matrix, dev, host, level_seed, mg_hierarchy, observation_matrix

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
CHILD_TIMEOUT = 600  # s; the child takes well under a minute
ARG_OUTOFRANGE, ARG_WRONGSTATE, SUP = 63, 73, 56
LRC_ENV = ("PMG_LRC_FUSED", "PMG_LRC_RESTORE", "PMG_LRC_REDUCE", "PMG_LRC_BTY", "PMG_LRC_BATCH", "PMG_LRC_DENSE")
ROWS_PER_BLOCK = 1024  # support rows per block of the row-compact B^T y kernels (256 threads x PMG_LRC_RPT)


def rel(got, want):
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-300)


def _clear_lrc_env(monkeypatch, env=None):
    for key in LRC_ENV:
        monkeypatch.delenv(key, raising=False)
    for key, val in (env or {}).items():
        monkeypatch.setenv(key, val)


# ------------------------------------------------------------------------------------------------------------
# single-level samplers: every rank x storage form, one child process under the kernel trace
# ------------------------------------------------------------------------------------------------------------
def _profiler():
    return shutil.which("rocprofv3") or next((p for p in ("/opt/rocm/bin/rocprofv3",) if os.path.exists(p)), None)


def _read_trace(d):
    """[(kernel name, grid size x)] of every dispatch under d, in dispatch order"""
    files = sorted(Path(d).rglob("*kernel_trace.csv"))
    assert files, f"rocprofv3 wrote no kernel_trace.csv under {d}"
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"], int(r["Grid_Size_X"])) for r in csv.DictReader(fh)]
    return [(name, gx) for _, name, gx in sorted(rows)]


def _segments(trace):
    """the launches of every case of W.CASES: from behind the second lrc_gemm_small_kernel of its set_lowrank to the marker"""
    cuts = [i for i, (name, _) in enumerate(trace) if "lrc_gemm_small_kernel" in name]
    ends = [i for i, (name, _) in enumerate(trace) if "spin_kernel" in name]
    assert len(cuts) == 2 * len(W.CASES) and len(ends) == len(W.CASES), (len(cuts), len(ends), len(W.CASES))
    segs = [trace[cuts[2 * i + 1] + 1:ends[i]] for i in range(len(W.CASES))]
    assert all(cuts[2 * i + 1] < ends[i] < (cuts[2 * i + 2] if i + 1 < len(W.CASES) else len(trace)) for i in range(len(W.CASES)))
    return segs


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    """(results of the child, launches per case or None without rocprofv3)"""
    tmp = tmp_path_factory.mktemp("lrc_ranks")
    out, tdir = tmp / "single.npz", tmp / "trace"
    prof = _profiler()
    env = {k: v for k, v in os.environ.items() if not k.startswith("PMG_") or k == "PMG_LIBRARY"}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [str(HERE / "lrc_rank_workloads.py"), str(out)]
    if prof:
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", str(tdir), "--"] + cmd
    p = subprocess.run(cmd, env=env, cwd=str(HERE.parent), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0 and out.exists(), f"child exited with {p.returncode}; stderr:\n{p.stderr[-4000:]}"
    with np.load(out) as z:
        res = {k: z[k] for k in z.files}
    segs = None
    if prof:
        segs = dict(zip(W.CASES, _segments(_read_trace(tdir))))
        shutil.rmtree(tdir)
    return res, segs


def _support(*mats):
    return np.flatnonzero(sum(np.abs(m).sum(1) for m in mats) > 0)


def _grids(seg, pattern):
    return {gx for name, gx in seg if pattern in name}


def _blocks(gx, threads):
    """a launch's grid size in workgroups (the trace may give it in work-items)"""
    return gx // threads if gx % threads == 0 and gx >= threads else gx


def _check_path(seg, path, k, ns):
    names = {name for name, _ in seg}
    has = lambda pat: any(pat in n for n in names)
    if path == "dense":
        assert has("lrc_btx_partial_kernel") and has("lrc_axpy_cols_kernel"), names
        for pat in ("lrc_gather_rows", "lrc_btx_rows_partial", "lrc_btx_axpy_small", "lrc_rhs_rows", "lrc_axpy_rows"):
            assert not has(pat), pat
        return
    assert not has("lrc_btx_partial_kernel") and not has("lrc_axpy_cols_kernel"), names
    # the support size the oracle predicts: ceil(ns / 256) blocks gather the compact rows, ceil(ns / 1024) sum B^T y
    assert {_blocks(g, 256) for g in _grids(seg, "lrc_gather_rows_kernel")} == {math.ceil(ns / 256)}
    fused = path.endswith("_fused")
    one_group = path == "small_fused"
    assert has("lrc_rhs_rows_kernel") == fused
    assert has("lrc_btx_axpy_small_kernel") == one_group
    if one_group:
        assert not has("lrc_btx_rows_partial"), names
        return
    assert {_blocks(g, 256) for g in _grids(seg, "lrc_btx_rows_partial_kernel")} == {math.ceil(ns / ROWS_PER_BLOCK)}
    if fused:
        assert has("lrc_axpy_restore_rows_kernel"), names
    else:  # the noise term by lrc_axpy_rows_kernel; the repair's partial sums added by the update kernel up to k = 8
        assert has("lrc_axpy_rows_kernel") and has("lrc_btx_rows_partial_kernel<true>"), names
        assert has("lrc_reduce_axpy_rows_kernel") == (k <= 8)
        assert has("lrc_reduce_kernel") == (k > 8)


@pytest.mark.parametrize("sampler,k,path", W.CASES, ids=[W.case_key(*c).replace("/", "-") for c in W.CASES])
def test_single_level_sampler_matches_oracle(single, sampler, k, path):
    res, segs = single
    c = W.case_inputs(sampler, k, path)
    key = W.case_key(sampler, k, path)
    grid, B, S, b, y0, omega = c["grid"], c["B"], c["S"], c["b"], c["y0"], c["omega"]
    A = O.shifted_laplace(*grid, W.KAPPA)
    n = A.n
    if sampler == "grid":
        col = O.coloring_redblack(*grid)
        noise = lambda d: O.noise_grid(*grid, W.SEED, W.CTR0 + d)
    else:
        col = res[f"{key}/colors"]
        noise = lambda d: O.noise_rows(n, W.SEED, W.CTR0 + d)
    eta = lambda d: O.noise_rows(k, (W.SEED + ETA_TAG) & M64, W.CTR0 + d)
    Bb_f = O.lrc_build_correction(A, col, B, S, omega, O.SOR_FORWARD)
    Bb_b = O.lrc_build_correction(A, col, B, S, omega, O.SOR_BACKWARD)

    # the storage form this case is built for: the joint support of B, Bb_f, Bb_b against a quarter of the layout
    ns, ld = len(_support(B, Bb_f, Bb_b)), int(res[f"{key}/ld"])
    assert (ns > ld // 4) == (path == "dense"), (ns, ld)
    if path != "dense":
        assert (ns <= ROWS_PER_BLOCK) == path.startswith("small"), ns
    if segs is not None:
        _check_path(segs[(sampler, k, path)], path, k, ns)

    for sweep, scaled in W.sweep_settings(omega):
        want = O.lrc_mcsor_apply(A, col, B, Bb_f, Bb_b, b, y0, omega, sweep)
        assert rel(res[f"{key}/apply{sweep}"], want) < 1e-12, sweep
        want = O.lrc_gibbs_samples(A, col, B, S, b, y0, W.ITS, noise, eta, omega, sweep, scaled)
        assert rel(res[f"{key}/sample{sweep}"], want) < 1e-11, sweep
        assert np.array_equal(res[f"{key}/b{sweep}"], b), "the right-hand side must come back bit for bit"


def test_single_level_paths_were_traced(single):
    """the kernel paths above are pinned only under rocprofv3's trace"""
    if single[1] is None:
        pytest.skip("rocprofv3 not found: the kernel paths were not checked (the results were)")


# ------------------------------------------------------------------------------------------------------------
# re-setting the update on a live single-level sampler; rank arguments out of range
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", W.SAMPLERS)
def test_resetting_the_rank_on_a_live_sampler(monkeypatch, sampler):
    """k = 3, then 64, then 0 on one handle: each result is the oracle's for the rank in force (nothing sized by the first call)"""
    from parmgmc_amd import MCSOR, GridMCSOR
    from parmgmc_amd.capi import PMGError

    _clear_lrc_env(monkeypatch)
    grid = (33, 33, 33)
    A = O.shifted_laplace(*grid, W.KAPPA)
    n = A.n
    if sampler == "grid":
        s = GridMCSOR(*grid, W.KAPPA)
        col = O.coloring_redblack(*grid)
        noise = lambda d: O.noise_grid(*grid, 5, d)
    else:
        s = MCSOR(A.rowptr, A.colidx, A.vals).setup()
        col = s.get_coloring()
        noise = lambda d: O.noise_rows(n, 5, d)
    s.set_sweep_type(O.SOR_SYMMETRIC)
    rng = np.random.default_rng(3)
    b, y0 = rng.standard_normal(n), rng.standard_normal(n)
    for k in (3, 64, 0):
        if k:
            B, S = W.observations(grid, "balls", k, 77 + k)
        else:
            B, S = np.zeros((n, 0)), np.zeros(0)
        s.set_lowrank(B, S)
        bd, yd = dev(b), dev(y0)
        s.sample(bd, yd, 2, seed=5, counter0=0)
        if k:
            eta = lambda d: O.noise_rows(k, (5 + ETA_TAG) & M64, d)
            want = O.lrc_gibbs_samples(A, col, B, S, b, y0, 2, noise, eta, 1.0, O.SOR_SYMMETRIC, True)
            assert rel(host(yd), want) < 1e-11, k
        else:
            want = O.gibbs_samples(A, col, b, y0, 2, noise, 1.0, O.SOR_SYMMETRIC, True)
            assert rel(host(yd), want) < 1e-13
    from parmgmc_amd.capi import check, lib

    fn = lib.pmg_grid_set_lowrank if sampler == "grid" else lib.pmg_mcsor_set_lowrank
    Bm, Sm = np.ones((n, 65), order="F"), np.ones(65)
    for k in (-1, 65):  # the wrappers take k from B's shape: the entry point itself
        with pytest.raises(PMGError) as e:
            check(fn(s._h, k, Bm.ctypes.data, Sm.ctypes.data))
        assert e.value.code == ARG_OUTOFRANGE, k
    s.destroy()


@pytest.mark.parametrize("k", [64])
def test_chol_sampler_with_a_rank_64_update(k):
    """pmg_chol_create_csr_lowrank: the factor of the explicit sum A + B S B^T (src/pc_chols.c:119-153) and one sample"""
    from parmgmc_amd import CholSampler

    A = O.shifted_laplace(10, 9, 1, 2.0)
    B = observation_matrix(A.n, k, 21)
    B[:, W.ZERO_COLUMN] = 0.0
    S = np.linspace(5.0, 90.0, k)
    ch = CholSampler(A.rowptr, A.colidx, A.vals, B, S)
    L = O.potrf_lower(A.dense() + B @ np.diag(S) @ B.T)
    assert np.allclose(ch.factor(), L, rtol=1e-13, atol=1e-15)
    rng = np.random.default_rng(4)
    b = rng.standard_normal(A.n)
    y = dev(np.zeros(A.n))
    ch.sample(dev(b), y, seed=8, counter=3)
    want = O.chol_sample(L, b, O.noise_rows(A.n, 8, 3))
    assert rel(host(y), want) < 1e-12
    # the last column counts: its S changed by half moves the factor far outside the tolerance
    S2 = S.copy()
    S2[63] *= 1.5
    assert np.abs(ch.factor() - O.potrf_lower(A.dense() + B @ np.diag(S2) @ B.T)).max() > 1e-8


# ------------------------------------------------------------------------------------------------------------
# MGMC whole chains against the oracle
# ------------------------------------------------------------------------------------------------------------
def _mg_observations(grid, kind, k):
    if kind == "dense":  # every column on a third of the rows
        B, S = W.observations(grid, "wide", k, 40 + k)
        if k == 64:
            B[:, W.ZERO_COLUMN] = 0.0
        return B, S
    return W.observations(grid, "points", k, 50 + k)


# name -> (grid, levels, observations, nu, omega, sweep, scaled, coarse, coarse its, correction form, environment)
MG_CASES = {
    "compact_top_chol": ((17, 17, 9), 3, "points", 1, 1.0, O.SOR_FORWARD, False, "cholsampler", 1, False, {}),
    "compact_top_chol_literal": ((17, 17, 9), 3, "points", 1, 1.0, O.SOR_BACKWARD, False, "cholsampler", 1, True, {}),
    "dense_gibbs_symmetric": ((9, 9, 5), 3, "dense", 2, 1.2, O.SOR_SYMMETRIC, True, "gibbs", 2, False, {}),
    "sliced_ell_levels": ((17, 17, 9), 3, "points", 1, 1.0, O.SOR_SYMMETRIC, True, "gibbs", 1, False, {"PMG_MG_NO_STENCIL": "1"}),
}


def _level_forms(mg, levels):
    """per level: ('compact', ns), 'dense', or None (no update held by the level: the exact coarse sampler, sliced-ELL levels)"""
    from parmgmc_amd.capi import PMGError

    out = []
    for l in range(levels):
        try:
            out.append(("compact", len(mg.level_lowrank_factors(l)[0])))
        except PMGError as e:
            assert e.code in (SUP, ARG_WRONGSTATE), e
            out.append("dense" if e.code == SUP else None)
    return out


def _mgmc_vs_oracle(monkeypatch, name, k, S_oracle=None, eta_col=None):
    """(relative error against the oracle, level forms); S_oracle / eta_col: negative controls of the last column"""
    from parmgmc_amd import MGMC
    from parmgmc_amd.capi import PMGError

    grid, levels, kind, nu, omega, sweep, scaled, coarse, coarse_its, literal, env = MG_CASES[name]
    _clear_lrc_env(monkeypatch)
    monkeypatch.delenv("PMG_MG_NO_STENCIL", raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    lv = mg_hierarchy(grid, 2.0, levels)
    n = int(np.prod(grid))
    B, S = _mg_observations(grid, kind, k)
    rng = np.random.default_rng(12)
    b, y0 = rng.standard_normal(n), rng.standard_normal(n)
    mg = MGMC(*grid, 2.0, levels)
    mg.set_smoother(scaled, omega, sweep, nu)
    mg.set_coarse(coarse, coarse_its)
    mg.set_correction_form(literal)
    mg.set_lowrank(*W.observations(grid, "points", 3, 1))  # re-set before set-up: the last call counts
    mg.set_lowrank(B, S)
    mg.setup()
    with pytest.raises(PMGError) as e:  # ... and only before set-up
        mg.set_lowrank(B, S)
    assert e.value.code == ARG_WRONGSTATE
    forms = _level_forms(mg, levels)
    yd = dev(y0)
    seed, c0, its = 0xBEEF, 3, 2
    mg.sample(dev(b), yd, its, seed=seed, counter0=c0, guesszero=False)
    mg.destroy()
    top = levels - 1
    colors = [O.coloring_parity8(*x["dims"]) for x in lv]
    colors[top] = O.coloring_redblack(*grid)
    orc = LrcMgmcOracle(lv, colors, B, S if S_oracle is None else S_oracle, nu, omega, sweep, scaled, coarse, coarse_its)
    sizes = [x["A"].shape[0] for x in lv]

    def xi(it, l, c):
        ctr = 64 * (c0 + it) + c
        return O.noise_grid(*grid, level_seed(seed, l), ctr) if l == top else O.noise_rows(sizes[l], level_seed(seed, l), ctr)

    def eta(it, l, c):
        e = O.noise_rows(k, (level_seed(seed, l) + ETA_TAG) & M64, 64 * (c0 + it) + c)
        if eta_col is not None:  # this column's draw from a shifted counter
            e[eta_col] = O.noise_rows(k, (level_seed(seed, l) + ETA_TAG) & M64, 64 * (c0 + it) + c + 1)[eta_col]
        return e

    chol_xi = lambda it: O.noise_rows(sizes[0], level_seed(seed, 0), 64 * (c0 + it))
    want = orc.chain(b, y0, its, False, xi, eta, chol_xi)
    return rel(host(yd), want), forms


@pytest.mark.parametrize("k", W.RANKS)
@pytest.mark.parametrize("name", list(MG_CASES))
def test_mgmc_chain_matches_oracle(monkeypatch, name, k):
    err, forms = _mgmc_vs_oracle(monkeypatch, name, k)
    grid, levels, kind = MG_CASES[name][:3]
    top = levels - 1
    if kind == "points":  # one grid point per observation: at most 7 support rows a column on the grid level
        assert forms[top][0] == "compact" and 0 < forms[top][1] <= 7 * k, forms
    else:
        assert forms[top] == "dense", forms
    if MG_CASES[name][-1].get("PMG_MG_NO_STENCIL"):
        assert all(f is None for f in forms[:top]), forms  # the sliced-ELL samplers hold their updates themselves
    else:
        assert all(f is not None for f in forms[1:]), forms
        assert (forms[0] is None) == (MG_CASES[name][7] == "cholsampler"), forms
    assert err < 1e-10, (err, forms)


@pytest.mark.parametrize("name", ["compact_top_chol", "dense_gibbs_symmetric"])
def test_mgmc_negative_control_of_the_last_column(monkeypatch, name):
    """the 64th column's contribution cannot hide inside the tolerance: the device misses an oracle whose S[63] is 1.5x, or
    whose eta[63] comes from the next counter, by more than 100x the tolerance"""
    k = 64
    S = _mg_observations(MG_CASES[name][0], MG_CASES[name][2], k)[1].copy()
    S[63] *= 1.5
    err, _ = _mgmc_vs_oracle(monkeypatch, name, k, S_oracle=S)
    assert err > 100 * 1e-10, err
    err, _ = _mgmc_vs_oracle(monkeypatch, name, k, eta_col=63)
    assert err > 100 * 1e-10, err


# ------------------------------------------------------------------------------------------------------------
# MGMC at 65^3: several blocks of support rows; each low-rank step once against numpy on the device's factors
# ------------------------------------------------------------------------------------------------------------
def _balls(grid, k, target, seed, spread=0.3):
    """k balls of about target / k grid points each, centred within spread of the middle; one of them empty at k = 64"""
    rng = np.random.default_rng(seed)
    r = (target / k / (4.19 * (grid[0] - 1) * (grid[1] - 1) * (grid[2] - 1))) ** (1 / 3)
    centres = [tuple(rng.uniform(0.5 - spread, 0.5 + spread, 3)) for _ in range(k)]
    radii = list(rng.uniform(0.9 * r, 1.1 * r, k))
    if k == 64:
        radii[W.ZERO_COLUMN] = 0.0
    B = ball_matrix(grid, centres, radii)
    assert np.count_nonzero(np.abs(B).sum(0)) == k - (k == 64)
    return B, rng.uniform(20.0, 90.0, k)


@pytest.mark.parametrize("k", W.RANKS)
def test_mgmc_lowrank_steps_on_many_blocks(monkeypatch, k):
    import torch

    from parmgmc_amd import MGMC, GridMCSOR

    _clear_lrc_env(monkeypatch)
    grid, levels = (65, 65, 65), 4
    top = levels - 1
    B, S = _balls(grid, k, 2500.0, 300 + k, spread=0.15)  # close together: the next level's support stays row-compact too
    mg = MGMC(*grid, 2.0, levels)
    mg.set_lowrank(B, S)
    mg.setup()
    g = GridMCSOR(*grid, 2.0)
    kind, ld, _ = mg.level_layout(top)
    iota = torch.arange(1, g.n + 1, dtype=torch.float64, device="cuda")
    nat_of_pos = g.to_cvec(iota).cpu().numpy().astype(np.int64) - 1
    assert kind == 0 and ld == len(nat_of_pos)
    rows, Bl, Bf, Bb = mg.level_lowrank_factors(top)
    assert ROWS_PER_BLOCK < len(rows) < ld // 4, len(rows)  # row-compact, several blocks
    nat = nat_of_pos[rows]
    assert (nat >= 0).all() and np.array_equal(Bl, B[nat, :])
    assert np.isin(_support(B), nat).all()
    rows1, B1, B1f, _ = mg.level_lowrank_factors(top - 1)  # the class-stencil level below: row-compact too
    kind1, ld1, _ = mg.level_layout(top - 1)
    assert kind1 == 1 and 0 < len(rows1) < ld1 // 4
    if k == 64:
        assert not Bl[:, W.ZERO_COLUMN].any() and not Bf[:, W.ZERO_COLUMN].any() and not B1[:, W.ZERO_COLUMN].any()
    out = np.ones(ld, bool)
    out[rows] = False
    out1 = np.ones(ld1, bool)
    out1[rows1] = False

    gen = torch.Generator(device="cuda").manual_seed(7 + k)
    y = torch.randn(ld, dtype=torch.float64, device="cuda", generator=gen)
    yh = y.cpu().numpy()
    # y -= Bb (B^T y): on a random y (untouched rows bit-equal), and on a y that is zero but for one row inside every ball,
    # where the correction shows without cancellation
    live = [c for c in range(k) if Bl[:, c].any()]
    hot = sorted({int(np.flatnonzero(Bl[:, c])[len(np.flatnonzero(Bl[:, c])) // 2]) for c in live})
    cold = np.ones(len(rows), bool)
    cold[hot] = False
    for backward, Bx in ((False, Bf), (True, Bb)):
        y2 = y.clone()
        mg.level_lowrank_post(top, y2, backward=backward)
        got = y2.cpu().numpy()
        want = yh[rows] - Bx @ (Bl.T @ yh[rows])
        assert np.array_equal(got[out], yh[out]) and rel(got[rows], want) < 1e-13
        ys = np.zeros(ld)
        ys[rows[hot]] = 1.0 + np.arange(len(hot))
        y3 = dev(ys)
        mg.level_lowrank_post(top, y3, backward=backward)
        corr = Bx @ (Bl.T @ ys[rows])
        assert np.abs(corr[cold]).max() > 0 and rel(-host(y3)[rows][cold], corr[cold]) < 1e-13, backward
    # r -= B (S o B^T x), plain and restricted to the next level (b_c -= B_c (S o B^T x)); the term alone on zero vectors
    wk = S * (Bl.T @ yh[rows])
    r = torch.randn(ld, dtype=torch.float64, device="cuda", generator=gen)
    rh = r.cpu().numpy()
    mg.level_lowrank_residual_sub(top, y, r, restricted=False)
    got = r.cpu().numpy()
    assert np.array_equal(got[out], rh[out]) and rel(got[rows], rh[rows] - Bl @ wk) < 1e-13
    rz = torch.zeros(ld, dtype=torch.float64, device="cuda")
    mg.level_lowrank_residual_sub(top, y, rz, restricted=False)
    assert not rz.cpu().numpy()[out].any() and rel(-rz.cpu().numpy()[rows], Bl @ wk) < 1e-12
    bz = torch.zeros(ld1, dtype=torch.float64, device="cuda")
    mg.level_lowrank_residual_sub(top, y, bz, restricted=True)
    term = -bz.cpu().numpy()
    assert not term[out1].any() and rel(term[rows1], B1 @ wk) < 1e-12
    # the class-stencil level's own repair
    y1 = torch.randn(ld1, dtype=torch.float64, device="cuda", generator=gen)
    y1h = y1.cpu().numpy()
    mg.level_lowrank_post(top - 1, y1, backward=False)
    got = y1.cpu().numpy()
    assert np.array_equal(got[out1], y1h[out1]) and rel(got[rows1], y1h[rows1] - B1f @ (B1.T @ y1h[rows1])) < 1e-13
    mg.destroy()
    del g, y, r, rz, bz, y1
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------
# folds and fused forms that are claimed to give the same bits, beyond k = 11
# ------------------------------------------------------------------------------------------------------------
def _vcycle_chain(monkeypatch, env, grid, levels, B, S, b, y0, sweep, its):
    from parmgmc_amd import MGMC

    _clear_lrc_env(monkeypatch, env)
    mg = MGMC(*grid, 2.0, levels)
    mg.set_smoother(True, 1.0, sweep, 1)
    mg.set_lowrank(B, S)
    mg.setup()
    ns = len(mg.level_lowrank_factors(levels - 1)[0])
    bd, yd = dev(b), dev(y0)
    mg.sample(bd, yd, its, seed=23, counter0=0)
    assert np.array_equal(host(bd), b), "the right-hand side must come back bit for bit"
    mg.destroy()
    return host(yd).copy(), ns


@pytest.mark.parametrize("k", [9, 64])
@pytest.mark.parametrize("sweep", [O.SOR_FORWARD, O.SOR_SYMMETRIC])
def test_folds_and_fused_forms_equal_the_default_bit_for_bit(monkeypatch, k, sweep):
    """65 x 65 x 33, 4 levels, several blocks of support rows on the finest level: the default against the switched-off
    restore, reduction and batched noise draw (one at a time and all together) and against PMG_LRC_FUSED=1.  At k = 64 the
    batched draw fills its 64-number slots exactly."""
    grid, levels = (65, 65, 33), 4
    n = int(np.prod(grid))
    B, S = _balls(grid, k, 5000.0, 500 + k)
    rng = np.random.default_rng(100 + k)
    b, y0 = rng.standard_normal(n), rng.standard_normal(n)
    want, ns = _vcycle_chain(monkeypatch, {"PMG_LRC_RESTORE": "0", "PMG_LRC_REDUCE": "0", "PMG_LRC_BATCH": "0"}, grid, levels, B, S, b, y0, sweep, 3)
    assert 4 * ROWS_PER_BLOCK < ns < n // 6, ns
    assert np.isfinite(want).all()
    for env in ({}, {"PMG_LRC_BATCH": "0"}, {"PMG_LRC_REDUCE": "0"}, {"PMG_LRC_RESTORE": "0"}, {"PMG_LRC_FUSED": "1"}):
        got, ns2 = _vcycle_chain(monkeypatch, env, grid, levels, B, S, b, y0, sweep, 3)
        assert ns2 == ns and np.array_equal(got, want), env
