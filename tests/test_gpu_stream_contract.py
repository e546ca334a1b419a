"""The stream contract of include/parmgmc_hip.h ("All device work is enqueued on `stream` and NOT synchronised") on
non-default streams, for every single-device entry point that takes a stream.  Every comparison is torch.equal /
np.array_equal against the same calls on the default stream; the deterministic sweeps and residuals are also compared
with the oracle, so the module does not rest on the library alone.

  first use      a fresh handle makes its very first device call on a side stream (torch side streams are non-blocking:
                 not ordered against the null stream), chains handles the sequence C = 3, C = 65 (workspace growth), C = 3
                 with other seeds (key upload), the per-chain right-hand-side form (its buffer on a warm handle) -- no host
                 synchronisation in between; a twin handle makes the same calls on the default stream
  slow producer  steady state (warm handle, same C, same seeds): the inputs hold NaN until copies that sit behind a delay on
                 the side stream overwrite them; a launch that is not ordered behind the stream's queue reads NaN.  Two
                 clones on a third stream (after the producer is queued, after the call returned) must still see NaN,
                 otherwise the case FAILS with "delay too short" -- it cannot pass vacuously
  capture        the same steady-state calls captured into a graph on a side stream and replayed on new data: a launch
                 outside the captured stream is missing from the replay
  two handles    two handles on two streams, calls interleaved from the host: process-global scratch would mix them

Delay: DELAY_REPS float64 products of two DELAY_N x DELAY_N matrices (1.4e11 flop each: at least 1.7 ms at the 79 Tflop/s
float64 peak of the MI355X, so 24 of them at least 40 ms).  The slow-producer test prints, per case, the host time of one call
on an idle stream (perf_counter) and the length of the delay (events); run it with -s.  Measured on an MI355X: enqueue
0.015 ms (CholSampler.sample) to 0.144 ms (AIJ MGMC.sample_chains, Gibbs coarse level), 0.03 ms for GridMCSOR.sample,
0.08 - 0.13 ms for the MCSOR, geometric MGMC and Woodbury calls; delay 44 - 49 ms, i.e. 300 times the longest enqueue time.

The third stream of the slow-producer test must run beside the side stream: a process has only a few hardware queues, and two
streams that share one run one after the other, so that a clone on the second waits for the delay on the first.  The
`streams` fixture tries stream pairs until a probe on one finishes while the delay on the other is still running.

Found with this module and fixed in pmg_common.c: hipMemset, with which pmg_dev_alloc zero-fills, runs on the null stream
and can finish after the call has returned; kernels the caller's non-blocking stream ran next on a buffer made lazily (the
grid's scratch cvecs, the chains workspaces) could be overwritten by the late zero fill.  test_first_use_grid and
test_two_handles_two_streams[mgmc_aij_sample_chains_chol] failed intermittently before pmg_dev_zero waited for the fill.

Left out: the distributed objects (pmg_dist*, pmg_distmcsor*, row blocks), which own a comm stream and need several
processes, and PCPARSOR.  PC types mcgibbs and gamgmc have no apply, cholsampler has no applyrichardson (as in the reference);
the test records the status of the missing operation instead."""
import contextlib
import gc
import time
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

import oracle as O

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
SEEDS = [0xFACE + 1013 * c for c in range(80)]
DELAY_N, DELAY_REPS = 4096, 24
NOT_SUPPORTED = 56


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


# ---- operators ------------------------------------------------------------------------------------------------------------
def random200():
    """the random200 matrix of test_gpu_chains.py"""
    rng = np.random.default_rng(1)
    M = sp.random(200, 200, density=0.03, random_state=rng, format="csr")
    M = M + M.T
    M = M + sp.diags(np.abs(M).sum(axis=1).A1 + 1.0)
    return O.CSR.from_scipy(M)


def galerkin27():
    return O.CSR.from_scipy(O.galerkin(O.shifted_laplace(9, 9, 9, 1.0).scipy(), O.q1_interp(5, 5, 5)))


def observations(n, k, form, seed):
    """B (n x k), S: the two storage forms of observations_17 (test_gpu_lowrank_chains.py) on any row count -- wide: every
    column on a third of the rows (dense form); rows: the columns on two sets of n / 12 rows (row-compact form)"""
    rng = np.random.default_rng(seed)
    B = np.zeros((n, k))
    sets = [rng.choice(n, size=max(n // 12, 2), replace=False) for _ in range(2)]
    for j in range(k):
        idx = rng.choice(n, size=n // 3, replace=False) if form == "wide" else sets[j % 2]
        B[idx, j] = rng.uniform(0.5, 1.5, len(idx)) / len(idx)
    return B, rng.uniform(20.0, 90.0, k)


MCSOR_CASES = {
    "lap6x5x4": (lambda: O.shifted_laplace(6, 5, 4, 2.0), None),
    "random200": (random200, None),
    "lap6x5x4_k3": (lambda: O.shifted_laplace(6, 5, 4, 2.0), "rows"),
    "random200_k3": (random200, "wide"),
}
GRIDS = {"33x7x3": (33, 7, 3, 0.5), "xtail257x5x3": (257, 5, 3, 10.0), "xcd12x61x5": (12, 61, 5, 2.0)}


def make_mcsor(name):
    from parmgmc_amd import MCSOR

    mk, form = MCSOR_CASES[name]
    A = mk()
    mc = MCSOR(A.rowptr, A.colidx, A.vals).setup()
    if form:
        mc.set_lowrank(*observations(A.n, 3, form, 31))
    return A, mc


@pytest.fixture(scope="module")
def aij():
    """lshape.msh refined twice, P1 kappa^2 M + K, aggregation hierarchy with coarse_max = 2000: two levels (1549, 6033 rows)"""
    from parmgmc_amd.unstructured import assemble_p1, build_hierarchy, read_gmsh41_triangles, refine_uniform

    xy, tris = read_gmsh41_triangles(GOLD / "lshape.msh")
    for _ in range(2):
        xy, tris = refine_uniform(xy, tris)
    A = assemble_p1(xy, tris, 1.0)
    ops, ps = build_hierarchy(A, coarse_max=2000)
    assert [len(o[0]) - 1 for o in ops] == [1549, 6033]
    return ops, ps


@pytest.fixture(scope="module")
def ex6():
    """the ~1000-row ex6 operator and its aggregation hierarchy (small enough for a dense reference covariance)"""
    from parmgmc_amd.unstructured import build_hierarchy

    A = O.ex6_matrix(32, 1e-2)
    ops, ps = build_hierarchy(A.scipy().tocsr(), coarse_max=100)
    assert len(ops) >= 2
    return A, ops, ps


def make_aij_mgmc(hier, coarse):
    from parmgmc_amd import COLORING_ITERATED, MGMC

    mg = MGMC.from_hierarchy(*hier)
    mg.set_coloring(COLORING_ITERATED)
    mg.set_smoother(True, 1.0, 1, 1)
    mg.set_coarse(coarse, 1)
    return mg.setup()


def make_woodbury(state):
    """PCWOODBURY on the Gibbs sampler of lap6x5x4 (MCSOR), Jacobi as the set-up solver (bit identity does not need a good one)"""
    from parmgmc_amd.wrappers import WoodburySampler

    A, mc = make_mcsor("lap6x5x4")
    dinv = dev(1.0 / A.scipy().diagonal())
    B, S = observations(A.n, 3, "rows", 32)
    wb = WoodburySampler(B, S, lambda b, x: x.copy_(b * dinv), lambda w, y, ctr: mc.sample(w, y, 1, state["seed"], counter0=ctr),
                         sample_chains=lambda W, Y, ctr: mc.sample_chains(W, Y, 1, state["seeds"], counter0=ctr))
    return A, mc, wb


# ---- the calls of one handle kind: script(handle, x, keep) -> {name: result}; every tensor it makes goes to keep -------------
def _cloner(keep):
    def new(t):
        keep.append(t.clone())
        return keep[-1]

    return new


def _zeros(keep, n):
    import torch

    keep.append(torch.zeros(n, dtype=torch.float64, device="cuda"))
    return keep[-1]


def chains_inputs(n, rng, sizes=(3, 65)):
    x = {"b": rng.standard_normal(n), "y": rng.standard_normal(n)}
    for c in sizes:
        x[f"Y{c}"] = rng.standard_normal((n, c))
        x[f"B{c}"] = rng.standard_normal((n, c))
    return x


def mcsor_script(mc, x, keep, lowrank=False):
    from parmgmc_amd.capi import check, lib
    from parmgmc_amd.wrappers import _ptr, _stream

    new, out = _cloner(keep), {}
    # the chains sequence first: every chains buffer is made inside these calls
    for tag, c, seeds in (("chains3", 3, SEEDS[:3]), ("chains65", 65, SEEDS[:65]), ("chains3_reseeded", 3, SEEDS[70:73])):
        out[tag] = new(x[f"Y{c}"])
        out[tag + "_ctr"] = mc.sample_chains(x["b"], out[tag], 2, seeds, counter0=5)
    for c in (3, 65):
        out[f"chains_rhs{c}"] = new(x[f"Y{c}"])
        mc.sample_chains(x[f"B{c}"], out[f"chains_rhs{c}"], 2, SEEDS[70:70 + c] if c == 3 else SEEDS[:65], counter0=5)
    out["apply_chains"] = new(x["Y3"])
    mc.apply_chains(x["b"], out["apply_chains"])
    out["apply"] = new(x["y"])
    mc.apply(x["b"], out["apply"])
    out["sample"] = new(x["y"])
    out["sample_ctr"] = mc.sample(x["b"], out["sample"], 2, seed=0xBEEF, counter0=3)
    out["residual"] = _zeros(keep, mc.n)
    mc.residual(x["b"], x["y"], out["residual"])
    ld, s = mc.layout_len(), _stream()
    bl, yl, rl = (_zeros(keep, ld) for _ in range(3))
    check(lib.pmg_mcsor_to_layout(mc._h, _ptr(x["b"]), _ptr(bl), s))
    check(lib.pmg_mcsor_to_layout(mc._h, _ptr(x["y"]), _ptr(yl), s))
    check(lib.pmg_mcsor_apply_layout(mc._h, _ptr(bl), _ptr(yl), s))
    out["apply_layout"] = new(yl)
    check(lib.pmg_mcsor_sample_layout(mc._h, _ptr(bl), _ptr(yl), 2, 1, 0xBEEF, 9, None, s))
    check(lib.pmg_mcsor_residual_layout(mc._h, _ptr(bl), _ptr(yl), _ptr(rl), s))
    out["residual_layout"] = rl
    if not lowrank:  # the per-colour sweeps do not carry the low-rank repair
        for colour in range(mc.get_num_colors()):
            mc.sweep_color_layout(colour, bl, yl, noisy=True, scaled=True, seed=0xD00D, counter=4)
    out["from_layout"] = _zeros(keep, mc.n)
    check(lib.pmg_mcsor_from_layout(mc._h, _ptr(yl), _ptr(out["from_layout"]), s))
    return out


def grid_script(g, x, keep):
    new, out = _cloner(keep), {}
    out["apply"] = new(x["y"])
    g.apply(x["b"], out["apply"])
    out["sample"] = new(x["y"])
    out["sample_ctr"] = g.sample(x["b"], out["sample"], 2, seed=0xCAFE, counter0=1)
    bc, yc, rc = (_zeros(keep, g.cvec_len) for _ in range(3))
    g.to_cvec(x["b"], bc)
    g.to_cvec(x["y"], yc)
    g.residual_cvec(bc, yc, rc)
    out["residual"] = _zeros(keep, g.n)
    g.from_cvec(rc, out["residual"])
    g.apply_cvec(bc, yc)
    out["apply_cvec"] = new(yc)
    g.sample_cvec(bc, yc, 2, seed=0xCAFE, counter0=7)
    out["sample_cvec"] = new(yc)
    for colour in (0, 1):
        g.sweep_color_cvec(colour, bc, yc, noisy=True, seed=3, counter=2)
    g.sweep_color_planes_cvec(0, 1, g.nz - 1, bc, yc, noisy=True, seed=3, counter=5)
    g.sweep_color_planes_cvec(1, 0, 1, bc, yc)
    out["colour_sweeps"] = _zeros(keep, g.n)
    g.from_cvec(yc, out["colour_sweeps"])
    return out


def chol_script(ch, x, keep):
    new, out = _cloner(keep), {}
    out["sample"] = new(x["y"])
    ch.sample(x["b"], out["sample"], seed=5, counter=2)
    out["mean"] = new(x["y"])
    ch.sample(x["b"], out["mean"], noisy=False)
    return out


def _level_vec(mg, level, keep, gen):
    """a random vector in the layout of one level of a geometric hierarchy (pads zero, as the hierarchy keeps them)"""
    import torch

    from parmgmc_amd import GridMCSOR

    kind, ld, off = mg.level_layout(level)
    dims = mg.level_dims(level)
    n = dims[0] * dims[1] * dims[2]
    nat = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    keep.append(nat)
    if kind == 0:
        g = GridMCSOR(*dims, 2.0)  # the cvec layout depends on the dimensions alone
        assert g.cvec_len == ld
        v = g.to_cvec(nat)
        keep.append(g)
    else:
        v = torch.zeros(ld, dtype=torch.float64, device="cuda")
        v[off:off + n] = nat
    keep.append(v)
    return v


def mgmc_geo_script(mg, x, keep):
    import torch

    from parmgmc_amd import PMGError

    new, out = _cloner(keep), {}
    out["sample"] = new(x["y"])
    out["sample_ctr"] = mg.sample(x["b"], out["sample"], 2, seed=7, counter0=1)
    out["guesszero"] = new(x["y"])
    mg.sample(x["b"], out["guesszero"], 2, seed=7, counter0=3, guesszero=True)
    seen = []
    out["callback"] = new(x["y"])
    mg.sample(x["b"], out["callback"], 3, seed=8, callback=lambda it, y: seen.append(new(y)))
    for i, s in enumerate(seen):
        out[f"callback_sample{i}"] = s
    assert len(seen) == 3
    gen = torch.Generator(device="cuda").manual_seed(11)
    top = mg.levels - 1
    for level in (top, top - 1):
        kind, ld, _ = mg.level_layout(level)
        b, v = _level_vec(mg, level, keep, gen), _level_vec(mg, level, keep, gen)
        if kind == 1:  # level_sweep: class-stencil levels only
            for tag, kw in (("forward", {}), ("backward", {"backward": True}), ("noisy", {"noisy": True, "seed": 0xBEEF, "counter": 3})):
                out[f"l{level}_sweep_{tag}"] = new(v)
                mg.level_sweep(level, b, out[f"l{level}_sweep_{tag}"], **kw)
        out[f"l{level}_residual"] = _zeros(keep, ld)
        mg.level_residual(level, b, v, out[f"l{level}_residual"])
        ldc = mg.level_layout(level - 1)[1]
        out[f"l{level}_restrict"] = _zeros(keep, ldc)
        mg.level_restrict(level, new(out[f"l{level}_residual"]), out[f"l{level}_restrict"])
        out[f"l{level}_residual_restrict"] = _zeros(keep, ldc)
        try:
            mg.level_residual_restrict(level, b, v, out[f"l{level}_residual_restrict"])
        except PMGError as e:  # decided on the host before any launch: the cycle runs the two steps on this level
            assert e.code == NOT_SUPPORTED, e
            out[f"l{level}_residual_restrict"] = "not supported"
        out[f"l{level}_prolong_add"] = new(v)
        mg.level_prolong_add(level, _level_vec(mg, level - 1, keep, gen), out[f"l{level}_prolong_add"])
    return out


def mgmc_aij_script(mg, x, keep):
    new, out = _cloner(keep), {}
    for tag, c, seeds in (("chains3", 3, SEEDS[:3]), ("chains65", 65, SEEDS[:65]), ("chains3_reseeded", 3, SEEDS[70:73])):
        out[tag] = new(x[f"Y{c}"])
        out[tag + "_ctr"] = mg.sample_chains(x["b"], out[tag], 2, seeds, counter0=3)
    for c in (3, 65):
        out[f"chains_rhs{c}"] = new(x[f"Y{c}"])
        mg.sample_chains(x[f"B{c}"], out[f"chains_rhs{c}"], 1, SEEDS[70:73] if c == 3 else SEEDS[:65], counter0=3, guesszero=True)
    mg.set_correction_form(True)
    out["literal"] = new(x["Y3"])
    mg.sample_chains(x["b"], out["literal"], 2, SEEDS[70:73], counter0=1)
    mg.set_correction_form(False)
    seen = []
    out["callback"] = new(x["Y3"])
    mg.sample_chains(x["b"], out["callback"], 2, SEEDS[70:73], callback=lambda it, Y: seen.append(new(Y)))
    for i, s in enumerate(seen):
        out[f"callback_sample{i}"] = s
    assert len(seen) == 2
    out["sample"] = new(x["y"])
    out["sample_ctr"] = mg.sample(x["b"], out["sample"], 2, seed=SEEDS[1], counter0=3)
    top = mg.levels - 1
    ld, ldc = mg.level_layout(top)[1], mg.level_layout(top - 1)[1]  # any vectors of the level's length serve: twins get the same
    lb, lx = _zeros(keep, ld), _zeros(keep, ld)
    lb[:mg.n], lx[:mg.n] = x["b"], x["y"]
    out["level_residual"] = _zeros(keep, ld)
    mg.level_residual(top, lb, lx, out["level_residual"])
    out["level_restrict"] = _zeros(keep, ldc)
    mg.level_restrict(top, new(out["level_residual"]), out["level_restrict"])
    out["level_prolong_add"] = new(lx)
    mg.level_prolong_add(top, out["level_restrict"], out["level_prolong_add"])
    return out


def woodbury_script(w, x, keep):
    _, _, wb, state = w
    new, out = _cloner(keep), {}
    for tag, c, seeds in (("chains3", 3, SEEDS[:3]), ("chains65", 65, SEEDS[:65]), ("chains3_reseeded", 3, SEEDS[70:73])):
        state["seeds"] = seeds
        out[tag] = new(x[f"Y{c}"])
        wb.run_chains(x["b"], out[tag], 2, seeds, counter0=2)
    state["seed"] = SEEDS[4]
    out["run"] = new(x["y"])
    wb.run(x["b"], out["run"], 2, SEEDS[4], counter0=2)
    return out


def pc_script(pc, x, keep):
    from parmgmc_amd import PMGError

    new, out = _cloner(keep), {}
    for name, fn in (("apply_richardson", lambda y: pc.apply_richardson(x["b"], y, 2)), ("apply", lambda y: pc.apply(x["b"], y)),
                     ("richardson_guesszero", lambda y: pc.apply_richardson(x["b"], y, 1, guesszero=True)), ("ksp_solve", lambda y: pc.ksp_solve(x["b"], y, 2, guess_nonzero=False))):
        out[name] = new(x["y"])
        try:
            fn(out[name])
        except PMGError as e:  # the type has no such operation (decided on the host, as PETSc's PCApply does)
            assert e.code == NOT_SUPPORTED and "does not have" in str(e), e
            out[name] = "not supported"
    assert any(not isinstance(v, str) for v in out.values())
    return out


# ---- running a script on a side stream and on the default stream -------------------------------------------------------------
def to_dev(x):
    return {k: dev(v) for k, v in x.items()}


def run_first_use(build, script, x, **kw):
    """(side, twin): the script's results from a fresh handle whose first device call is on a side stream, and from a twin
    handle on the default stream; one host synchronisation at the end of each"""
    import torch

    side_h, twin_h = build(), build()
    xs, xt = to_dev(x), to_dev(x)
    keep = []
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        side = script(side_h, xs, keep, **kw)
    st.synchronize()
    twin = script(twin_h, xt, keep, **kw)
    torch.cuda.synchronize()
    return side, twin, (side_h, twin_h, xs, xt, keep)


def assert_same(side, twin):
    import torch

    assert side.keys() == twin.keys()
    for k in side:
        if isinstance(side[k], torch.Tensor):
            assert bool(torch.isfinite(side[k]).all()), k
            assert torch.equal(side[k], twin[k]), k
        else:
            assert side[k] == twin[k], k


# ---- test 1: first use on a side stream ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MCSOR_CASES))
def test_first_use_mcsor(name):
    A = MCSOR_CASES[name][0]()
    lowrank = MCSOR_CASES[name][1] is not None
    x = chains_inputs(A.n, np.random.default_rng(1))
    side, twin, alive = run_first_use(lambda: make_mcsor(name)[1], mcsor_script, x, lowrank=lowrank)
    assert_same(side, twin)
    mc = alive[0]
    if not lowrank:  # the deterministic calls against the oracle
        want = O.mcsor_apply(A, mc.get_coloring(), x["b"], x["y"], 1.0, O.SOR_FORWARD)
        assert np.array_equal(host(side["apply"]), want)
        assert np.array_equal(host(side["apply_layout"])[mc.get_layout()], want)
        for c in range(3):
            assert np.array_equal(host(side["apply_chains"])[:, c], O.mcsor_apply(A, mc.get_coloring(), x["b"], x["Y3"][:, c], 1.0, O.SOR_FORWARD)), c


def csr_residual(A, b, y):
    """sequential row sums in storage order, as test_gpu_grid.py compares the grid residual"""
    want = np.empty(A.n)
    for i in range(A.n):
        s = 0.0
        for q in range(A.rowptr[i], A.rowptr[i + 1]):
            s = s + A.vals[q] * y[A.colidx[q]]
        want[i] = b[i] - s
    return want


@pytest.mark.parametrize("name", list(GRIDS))
def test_first_use_grid(name):
    from parmgmc_amd import GridMCSOR

    nx, ny, nz, kappa = GRIDS[name]
    A = O.shifted_laplace(nx, ny, nz, kappa)
    rng = np.random.default_rng(2)
    x = {"b": rng.standard_normal(A.n), "y": rng.standard_normal(A.n)}
    side, twin, _ = run_first_use(lambda: GridMCSOR(nx, ny, nz, kappa), grid_script, x)
    assert_same(side, twin)
    want = O.mcsor_apply(A, O.coloring_redblack(nx, ny, nz), x["b"], x["y"], 1.0, O.SOR_FORWARD)
    assert np.array_equal(host(side["apply"]), want)
    assert np.array_equal(host(side["residual"]), csr_residual(A, x["b"], x["y"]))


def test_first_use_chol():
    from parmgmc_amd import CholSampler

    A = galerkin27()
    rng = np.random.default_rng(3)
    x = {"b": rng.standard_normal(A.n), "y": rng.standard_normal(A.n)}
    side, twin, _ = run_first_use(lambda: CholSampler(A.rowptr, A.colidx, A.vals), chol_script, x)
    assert_same(side, twin)


GEO = {"17x9x9_chol": ((17, 9, 9), "cholsampler"), "33x17x17_chol": ((33, 17, 17), "cholsampler"), "33x17x17_gibbs": ((33, 17, 17), "gibbs")}


def make_geo(name):
    from parmgmc_amd import MGMC

    dims, coarse = GEO[name]
    mg = MGMC(*dims, 2.0, 3)
    mg.set_coarse(coarse, 2)
    return mg.setup()


@pytest.mark.parametrize("name", list(GEO))
def test_first_use_mgmc_geometric(name):
    n = int(np.prod(GEO[name][0]))
    rng = np.random.default_rng(4)
    x = {"b": rng.standard_normal(n), "y": rng.standard_normal(n)}
    side, twin, _ = run_first_use(lambda: make_geo(name), mgmc_geo_script, x)
    assert_same(side, twin)


@pytest.mark.parametrize("coarse", ["cholsampler", "gibbs"])
def test_first_use_mgmc_aij(aij, coarse):
    n = len(aij[0][-1][0]) - 1
    x = chains_inputs(n, np.random.default_rng(5))
    side, twin, _ = run_first_use(lambda: make_aij_mgmc(aij, coarse), mgmc_aij_script, x)
    assert_same(side, twin)


def test_first_use_woodbury():
    def build():
        state = {}
        return make_woodbury(state) + (state,)

    x = chains_inputs(120, np.random.default_rng(6))
    side, twin, _ = run_first_use(build, woodbury_script, x)
    assert_same(side, twin)


PC_TYPES = {"mcgibbs": {}, "sorgibbs": {}, "cholsampler": {}, "gamgmc": {"-gamgmc_pc_mg_levels": "3", "-gamgmc_mg_levels_pc_type": "mcgibbs"}}
PC_STREAM_STRIDE = 0xD1B54A32D192ED03  # seed of a PC = global seed + stride * (creation index + 1), include/parmgmc_hip.h


@pytest.mark.parametrize("pc_type", list(PC_TYPES))
def test_first_use_pc_layer(pc_type):
    """the 9 x 9 ex1 operator; the PC is set up inside its first apply, on the side stream.  Twins get equal noise: every PC draws
    from its own stream of the global seed, so the twin runs under the global seed that gives it the side PC's stream."""
    import torch

    from parmgmc_amd import pc as P

    P.initialize()
    P.options_clear()
    try:
        for k, v in PC_TYPES[pc_type].items():
            P.options_set_value(k, v)

        def build():
            pc = P.PC(pc_type)
            if pc_type == "cholsampler":  # needs the assembled matrix
                A = O.shifted_laplace(9, 9, 1, 10.0)
                pc.set_operators(P.Mat.csr(A.rowptr, A.colidx, A.vals))
            else:
                pc.set_operators(P.Mat.dmda(9, 9, 1, 10.0))
            pc.set_from_options()
            return pc

        rng = np.random.default_rng(7)
        xs = to_dev({"b": rng.standard_normal(81), "y": rng.standard_normal(81)})
        keep = []
        P.set_seed(0xCAFE)
        side_pc, twin_pc = build(), build()
        seed_side, seed_twin = side_pc.noise_state()[0], twin_pc.noise_state()[0]
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            side = pc_script(side_pc, xs, keep)
        st.synchronize()
        P.set_seed((0xCAFE + seed_side - seed_twin) % 2**64)
        assert twin_pc.noise_state() == (seed_side, 0)
        twin = pc_script(twin_pc, xs, keep)
        torch.cuda.synchronize()
        assert_same(side, twin)
        assert side_pc.noise_state()[1] == twin_pc.noise_state()[1] > 0
    finally:
        P.options_clear()
        P.set_seed(0xCAFE)


def test_first_use_chainstats_and_chaincov_callbacks(ex6):
    """ChainStats and ChainCov as the callback of MGMC.sample_chains, the first call of every handle on the side stream"""
    import torch

    from parmgmc_amd import ChainStats
    from parmgmc_amd.wrappers import ChainCov

    A, ops, ps = ex6
    n, nchains, its = A.n, 8, 3
    rng = np.random.default_rng(8)
    x = to_dev({"b": rng.standard_normal(n), "Y": rng.standard_normal((n, nchains))})
    w = rng.standard_normal(n)

    def run(keep):
        mg = make_aij_mgmc((ops, ps), "cholsampler")
        cs = ChainStats(n, nchains, [None, w], max_steps=its)
        cov = ChainCov.from_csr(A.rowptr, A.colidx, A.vals, nchains, max_steps=its)
        Ys, Yc = x["Y"].clone(), x["Y"].clone()
        mg.sample_chains(x["b"], Ys, its, SEEDS[:nchains], stats=cs)
        mg.sample_chains(x["b"], Yc, its, SEEDS[:nchains], cov=cov)
        mean, var = cs.fields()
        keep += [mg, cs, cov, Ys, Yc, mean, var]
        return {"Ys": Ys, "Yc": Yc, "mean": mean, "var": var}, cs, cov

    keep = []
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        side, cs_s, cov_s = run(keep)
    st.synchronize()
    twin, cs_t, cov_t = run(keep)
    torch.cuda.synchronize()
    assert_same(side, twin)
    assert torch.equal(side["Ys"], side["Yc"])
    assert cs_s.count() == cs_t.count() == (its, its * nchains)
    for q in range(2):
        assert np.array_equal(cs_s.trace(q), cs_t.trace(q)) and np.isfinite(cs_s.trace(q)).all()
    assert cov_s.count() == its and np.array_equal(cov_s.errors(), cov_t.errors()) and np.isfinite(cov_s.errors()).all()


# ---- steady-state calls: call(b, y) updates y in place; shapes of b and y -----------------------------------------------------
STEADY = ["mcsor_sample", "mcsor_sample_chains", "mcsor_sample_chains_rhs", "mcsor_k3_sample", "mcsor_k3_sample_chains", "grid_sample", "grid_sample_xtail", "grid_sample_xcd",
          "chol_sample", "mgmc_geo_sample", "mgmc_geo_sample_gibbs", "mgmc_aij_sample_chains_chol", "mgmc_aij_sample_chains_gibbs", "mgmc_aij_sample_chains_rhs", "woodbury_run", "woodbury_run_chains"]
CAPTURED = [s for s in STEADY if s != "woodbury_run"]
NC = 8  # chains of the steady-state calls


def make_steady(name, aij):
    """(call, shape of b, shape of y) on a fresh handle; the closure keeps the handle alive"""
    from parmgmc_amd import CholSampler, GridMCSOR

    if name.startswith("mcsor"):
        A, mc = make_mcsor("random200_k3" if "_k3_" in name else "random200")
        if name.endswith("chains_rhs"):
            return (lambda b, Y: mc.sample_chains(b, Y, 2, SEEDS[:NC], counter0=3)), (A.n, NC), (A.n, NC)
        if name.endswith("chains"):
            return (lambda b, Y: mc.sample_chains(b, Y, 2, SEEDS[:NC], counter0=3)), (A.n,), (A.n, NC)
        return (lambda b, y: mc.sample(b, y, 2, seed=0xBEEF, counter0=3)), (A.n,), (A.n,)
    if name.startswith("grid"):
        dims = GRIDS[{"grid_sample": "33x7x3", "grid_sample_xtail": "xtail257x5x3", "grid_sample_xcd": "xcd12x61x5"}[name]]
        g = GridMCSOR(*dims)
        return (lambda b, y: g.sample(b, y, 2, seed=0xCAFE, counter0=1)), (g.n,), (g.n,)
    if name == "chol_sample":
        A = galerkin27()
        ch = CholSampler(A.rowptr, A.colidx, A.vals)
        return (lambda b, y: ch.sample(b, y, seed=5, counter=2)), (A.n,), (A.n,)
    if name.startswith("mgmc_geo"):
        mg = make_geo("33x17x17_gibbs" if name.endswith("gibbs") else "17x9x9_chol")
        return (lambda b, y: mg.sample(b, y, 2, seed=7, counter0=1)), (mg.n,), (mg.n,)
    if name.startswith("mgmc_aij"):
        mg = make_aij_mgmc(aij, "gibbs" if name.endswith("gibbs") else "cholsampler")
        bshape = (mg.n, NC) if name.endswith("rhs") else (mg.n,)
        return (lambda b, Y: mg.sample_chains(b, Y, 2, SEEDS[:NC], counter0=2)), bshape, (mg.n, NC)
    state = {"seed": SEEDS[4], "seeds": SEEDS[:NC]}
    A, mc, wb = make_woodbury(state)
    if name == "woodbury_run":
        return (lambda b, y: wb.run(b, y, 2, SEEDS[4], counter0=1)), (A.n,), (A.n,)
    return (lambda b, Y: wb.run_chains(b, Y, 2, SEEDS[:NC], counter0=1)), (A.n,), (A.n, NC)


def steady_inputs(bshape, yshape, seed):
    rng = np.random.default_rng(seed)
    return dev(rng.standard_normal(bshape)), dev(rng.standard_normal(yshape))


@pytest.fixture(scope="module")
def delay():
    """enqueue() queues about 50 ms of ordinary torch work (see the module docstring) on the current stream"""
    import torch

    a = torch.randn((DELAY_N, DELAY_N), dtype=torch.float64, device="cuda") / DELAY_N**0.5
    scratch = torch.empty_like(a)

    def enqueue():
        for _ in range(DELAY_REPS):
            torch.mm(a, a, out=scratch)

    enqueue()  # loads the BLAS kernels
    torch.cuda.synchronize()
    return enqueue


@contextlib.contextmanager
def no_collection():
    """no cyclic garbage collection inside: one that frees the handle of an earlier test calls hipFree, which waits for the
    whole device -- a host synchronisation that is not the library call's"""
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        gc.enable()


@pytest.fixture(scope="module")
def streams(delay):
    """(side, third): two streams that run concurrently (see the module docstring)"""
    import torch

    side = torch.cuda.Stream()
    poison = torch.full((4096,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(16):
        third = torch.cuda.Stream()
        behind, beside = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(side):
            delay()
            behind.record()
        with torch.cuda.stream(third):
            seen = poison.clone()
            beside.record()
        beside.synchronize()
        concurrent = not behind.query()
        torch.cuda.synchronize()
        del seen
        if concurrent:
            return side, third
    pytest.fail("no two streams of this process run concurrently")


# ---- test 2: ordering behind a slow producer --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STEADY)
def test_ordered_behind_a_slow_producer(name, aij, delay, streams):
    import torch

    call, bshape, yshape = make_steady(name, aij)
    b, y0 = steady_inputs(bshape, yshape, 21)
    want = y0.clone()
    call(b, want)  # the default-stream result; the handle is warm from here on
    torch.cuda.synchronize()
    (st, third), idle = streams, torch.cuda.Stream()
    with torch.cuda.stream(idle):  # the host time of one call on an idle stream
        y_idle = y0.clone()
        idle.synchronize()
        t0 = time.perf_counter()
        call(b, y_idle)
        enqueue_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    assert torch.equal(y_idle, want)
    b_side, y_side = torch.full_like(b, float("nan")), torch.full_like(y0, float("nan"))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with no_collection(), torch.cuda.stream(st):
        e0.record()
        delay()
        e1.record()
        b_side.copy_(b)
        y_side.copy_(y0)
        with torch.cuda.stream(third):
            seen_queued = b_side.clone()
        call(b_side, y_side)
        with torch.cuda.stream(third):
            seen_returned = b_side.clone()
    torch.cuda.synchronize()
    print(f"{name}: enqueue {enqueue_ms:.3f} ms, delay {e0.elapsed_time(e1):.1f} ms")
    assert bool(torch.isnan(seen_queued).all()), "delay too short: the poison was gone once the producer was queued"
    assert bool(torch.isnan(seen_returned).all()), "delay too short: the poison was gone when the call returned (or the call synchronises the host)"
    assert torch.equal(b_side, b)
    assert torch.equal(y_side, want)


# ---- test 3: capture and replay ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CAPTURED)
def test_capture_and_replay(name, aij):
    import torch

    call, bshape, yshape = make_steady(name, aij)
    b_static, y_static = steady_inputs(bshape, yshape, 22)
    b_new, y_new = steady_inputs(bshape, yshape, 23)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        call(b_static, y_static)  # warm on the capture stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        call(b_static, y_static)
    b_static.copy_(b_new)
    y_static.copy_(y_new)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want = y_new.clone()
    call(b_new, want)
    torch.cuda.synchronize()
    assert torch.equal(b_static, b_new)
    assert torch.equal(y_static, want)
    assert not torch.equal(want, y_new)


# ---- test 4: two handles on two streams -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mcsor_sample_chains", "grid_sample", "mgmc_aij_sample_chains_chol"])
def test_two_handles_two_streams(name, aij):
    import torch

    (call_a, bshape, yshape), (call_b, _, _) = make_steady(name, aij), make_steady(name, aij)
    ba, ya0 = steady_inputs(bshape, yshape, 24)
    bb, yb0 = steady_inputs(bshape, yshape, 25)
    ya, yb = ya0.clone(), yb0.clone()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    sa.wait_stream(torch.cuda.current_stream())
    sb.wait_stream(torch.cuda.current_stream())
    with no_collection():
        for _ in range(2):  # A, B, A, B: no host synchronisation in between
            with torch.cuda.stream(sa):
                call_a(ba, ya)
            with torch.cuda.stream(sb):
                call_b(bb, yb)
    torch.cuda.synchronize()
    for call, b, y0, got in ((call_a, ba, ya0, ya), (call_b, bb, yb0, yb)):  # every handle alone
        want = y0.clone()
        call(b, want)
        call(b, want)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
    assert not torch.equal(ya, yb)
