"""Child process of test_gpu_st27_splits.py: the kernels of the class-stencil levels of st27_splits.py in a fresh process (the
PMG_* switches are read once per process), EVERY ROW compared with the oracle here, the raw float64 vectors written to an .npz
for the parent's bit comparison between the switch settings.

    python st27_split_workloads.py <out.npz>

A failed comparison raises: the child exits non-zero and the parent reports its stderr.  Every figure that is held to a
tolerance is printed before it is checked."""
import functools
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
for p in (str(ROOT), str(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import st27_splits as M  # noqa: E402

KAPPA = 1.5
SEED_BIG = (1 << 40) + 0xBEEF  # above 2^32
COUNTER = 5
SMOOTHERS = [(False, 1.0), (True, 1.3)]  # (scaled, omega) of MGMC.set_smoother
NOISE_TOL = 1e-13  # of the largest entry: device log / sincos against glibc (test_gpu_fullsize_oracle.py)
TABLE_TOL = 1e-13  # of the largest entry: Galerkin sums in another order (test_hierarchy_matches_oracle)
VCYCLE_ITS = 3
VCYCLE_SEED, VCYCLE_COUNTER0 = 0xC0DE, 4
PAD = 3.0  # what the pad and ghost entries of an output vector hold before the kernel runs


def key(dims):
    return "x".join(map(str, dims))


def vcycle_inputs(grid):
    n = int(np.prod(grid))
    rng = np.random.default_rng(n)
    return rng.standard_normal(n), rng.standard_normal(n)


def need(cond, what):
    if not cond:
        raise AssertionError(what)


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def _host(t):
    return t.detach().cpu().numpy().copy()


def _padded(v, ld, off, fill=0.0):
    import torch

    out = torch.full((ld,), fill, dtype=torch.float64, device="cuda")
    out[off:off + len(v)] = _dev(v)
    return out


def _pads_hold(vec, off, n, fill):
    return bool((vec[:off] == fill).all() and (vec[off + n:] == fill).all())


def _mgmc(grid, levels, scaled, omega):
    from parmgmc_amd import MGMC

    mg = MGMC(*grid, KAPPA, levels)
    mg.set_smoother(scaled, omega, 1, 1)
    mg.set_coarse("gibbs", 1)  # the coarsest level is a class-stencil level too
    return mg.setup()


def level_kernels(out, tag, mg, level, dims, omega):
    """forward and backward sweeps without and with noise and the residual of one class-stencil level, every row"""
    import oracle as O

    cx, cy, cz = dims
    N = cx * cy * cz
    kind, ld, off = mg.level_layout(level)
    need(kind == 1 and off == cx * cy and ld == cx * cy * (cz + 2) and mg.level_dims(level) == dims, f"{tag}: layout {kind, ld, off} of level {mg.level_dims(level)}")
    coef, sqrtd = mg.level_stencil(level)
    rng = np.random.default_rng(N + int(10 * omega))
    b, y0 = rng.standard_normal(N), rng.standard_normal(N)
    rows = np.arange(N, dtype=np.int64)
    bp = _padded(b, ld, off)
    out[f"{tag}/in/coef"], out[f"{tag}/in/sqrtd"], out[f"{tag}/in/b"], out[f"{tag}/in/y0"] = coef, sqrtd, b, y0
    for backward in (False, True):
        d = "bwd" if backward else "fwd"
        yp = _padded(y0, ld, off)
        mg.level_sweep(level, bp, yp, backward=backward)
        y1 = _host(yp)
        want = O.st27_rows_sweep(cx, cy, cz, coef, sqrtd, rows, b, y0, y1[off:off + N], omega=omega, backward=backward)
        bad = np.nonzero(y1[off:off + N] != want)[0]
        need(not len(bad), f"{tag}: deterministic {d} sweep: {len(bad)} of {N} rows differ from the oracle, first {bad[:8]} (x = {bad[:8] % cx})")
        need(_pads_hold(y1, off, N, 0.0), f"{tag}: deterministic {d} sweep wrote a ghost plane")
        out[f"{tag}/det_{d}"] = y1
        yp = _padded(y0, ld, off)
        mg.level_sweep(level, bp, yp, backward=backward, noisy=True, seed=SEED_BIG, counter=COUNTER)
        y1 = _host(yp)
        want = O.st27_rows_sweep(cx, cy, cz, coef, sqrtd, rows, b, y0, y1[off:off + N], omega=omega, backward=backward, noisy=True, seed=SEED_BIG, sweep=COUNTER)
        err = float(np.abs(y1[off:off + N] - want).max()) / float(np.abs(want).max())
        print(f"{tag}: noisy {d} sweep {err:.3e}")
        need(err <= NOISE_TOL, f"{tag}: noisy {d} sweep is {err:.3e} of the largest entry from the oracle, row {int(np.abs(y1[off:off + N] - want).argmax())}")
        need(_pads_hold(y1, off, N, 0.0), f"{tag}: noisy {d} sweep wrote a ghost plane")
        out[f"{tag}/noisy_{d}"] = y1
    rp = _padded(np.zeros(N), ld, off, PAD)
    mg.level_residual(level, bp, _padded(y0, ld, off), rp)
    r = _host(rp)
    bad = np.nonzero(r[off:off + N] != O.st27_rows_residual(cx, cy, cz, coef, rows, b, y0))[0]
    need(not len(bad), f"{tag}: residual: {len(bad)} of {N} rows differ from the oracle, first {bad[:8]} (x = {bad[:8] % cx})")
    need(_pads_hold(r, off, N, PAD), f"{tag}: the residual wrote a ghost plane")
    out[f"{tag}/resid"] = r


@functools.lru_cache(maxsize=None)
def oracle_table(fine, dims):
    """the class table of the oracle's Galerkin operator of the level `dims` below the grid `fine`, and the classes it has"""
    import oracle as O

    A = O.galerkin(O.shifted_laplace(*fine, KAPPA).scipy(), O.q1_interp(*dims))
    want, have, exact = O.st27_table_from_csr(*dims, O.CSR.from_scipy(A))
    return want, have


def stencil_table(tag, mg, fine, dims, scaled, omega):
    coef, sqrtd = mg.level_stencil(0)
    want, have = oracle_table(fine, dims)
    top = float(np.abs(want).max())
    err = float(np.abs(coef[have] - want[have]).max()) / top
    print(f"{tag}: stencil table {err:.3e}, {int(have.sum())} classes")
    need(err <= TABLE_TOL, f"{tag}: stencil table {err:.3e} of the largest entry from the oracle's Galerkin product")
    need(int(have.sum()) == (27 if dims[2] > 2 else 18 if dims[2] == 2 else 9), f"{tag}: {int(have.sum())} position classes")
    sq = np.sqrt(np.abs(want[have, 13])) * (np.sqrt((2 - omega) / omega) if scaled else 1.0)
    need(float(np.abs(sqrtd[have] - sq).max()) <= TABLE_TOL * float(sq.max()), f"{tag}: noise scales")


def grid_transfers(out, tag, mg, top, fine, coarse, fused=True):
    """restriction, prolongation and the fused residual + restriction from the grid level `top` to the level below, every row"""
    import oracle as O
    from parmgmc_amd import GridMCSOR, PMGError

    nf, nc = int(np.prod(fine)), int(np.prod(coarse))
    g = GridMCSOR(*fine, KAPPA)
    kind, ld, _ = mg.level_layout(top)
    _, ldc, offc = mg.level_layout(top - 1)
    need(kind == 0 and ld == g.cvec_len and offc == coarse[0] * coarse[1], f"{tag}: layouts")
    rng = np.random.default_rng(nf)
    r, x0, e = rng.standard_normal(nf), rng.standard_normal(nf), rng.standard_normal(nc)
    crow, frow = np.arange(nc, dtype=np.int64), np.arange(nf, dtype=np.int64)
    bc = _padded(np.zeros(nc), ldc, offc, PAD)
    mg.level_restrict(top, g.to_cvec(_dev(r)), bc)
    got = _host(bc)
    bad = np.nonzero(got[offc:offc + nc] != O.q1_rows_restrict(fine, coarse, crow, r))[0]
    need(not len(bad), f"{tag}: restriction: {len(bad)} of {nc} rows differ, first {bad[:8]}")
    need(_pads_hold(got, offc, nc, PAD), f"{tag}: the restriction wrote a ghost plane")
    out[f"{tag}/restrict"] = got
    xc = g.to_cvec(_dev(x0))
    mg.level_prolong_add(top, _padded(e, ldc, offc), xc)
    got = _host(g.from_cvec(xc))
    bad = np.nonzero(got != O.q1_rows_prolong_add(fine, coarse, frow, x0, e))[0]
    need(not len(bad), f"{tag}: prolongation: {len(bad)} of {nf} rows differ, first {bad[:8]}")
    out[f"{tag}/prolong"] = got
    if fused:
        bc = _padded(np.zeros(nc), ldc, offc, PAD)
        try:
            mg.level_residual_restrict(top, g.to_cvec(_dev(r)), g.to_cvec(_dev(x0)), bc)
        except PMGError as err:  # the cycle runs the two steps there: only where a direction is not coarsened
            need(err.code == 56 and fine[2] == coarse[2], f"{tag}: no fused residual + restriction: {err}")
        else:
            need(fine[2] != coarse[2], f"{tag}: a fused residual + restriction on a semicoarsened level")
            got = _host(bc)
            want = O.q1_rows_restrict(fine, coarse, crow, O.grid7_rows_residual(*fine, KAPPA, frow, r, x0))
            bad = np.nonzero(got[offc:offc + nc] != want)[0]
            need(not len(bad), f"{tag}: fused residual + restriction: {len(bad)} of {nc} rows differ, first {bad[:8]}")
            need(_pads_hold(got, offc, nc, PAD), f"{tag}: the fused residual + restriction wrote a ghost plane")
            out[f"{tag}/fused_rr"] = got
    g.destroy()


def st27_transfers(out, tag, mg, level, fine, coarse):
    """restriction and prolongation between the class-stencil level `level` and the one below, every row"""
    import oracle as O

    nf, nc = int(np.prod(fine)), int(np.prod(coarse))
    _, ld, off = mg.level_layout(level)
    _, ldc, offc = mg.level_layout(level - 1)
    rng = np.random.default_rng(nf + 1)
    r, x0, e = rng.standard_normal(nf), rng.standard_normal(nf), rng.standard_normal(nc)
    bc = _padded(np.zeros(nc), ldc, offc, PAD)
    mg.level_restrict(level, _padded(r, ld, off), bc)
    got = _host(bc)
    bad = np.nonzero(got[offc:offc + nc] != O.q1_rows_restrict(fine, coarse, np.arange(nc, dtype=np.int64), r))[0]
    need(not len(bad), f"{tag}: restriction: {len(bad)} of {nc} rows differ, first {bad[:8]}")
    need(_pads_hold(got, offc, nc, PAD), f"{tag}: the restriction wrote a ghost plane")
    out[f"{tag}/restrict"] = got
    xp = _padded(x0, ld, off, 2.5)
    mg.level_prolong_add(level, _padded(e, ldc, offc), xp)
    got = _host(xp)
    bad = np.nonzero(got[off:off + nf] != O.q1_rows_prolong_add(fine, coarse, np.arange(nf, dtype=np.int64), x0, e))[0]
    need(not len(bad), f"{tag}: prolongation: {len(bad)} of {nf} rows differ, first {bad[:8]}")
    need(_pads_hold(got, off, nf, 2.5), f"{tag}: the prolongation wrote a ghost plane")
    out[f"{tag}/prolong"] = got


def tabled_shapes(out):
    for dims in M.SHAPES:
        fine = M.fine_grid(dims)
        for si, (scaled, omega) in enumerate(SMOOTHERS):
            mg = _mgmc(fine, 2, scaled, omega)
            tag = f"{key(dims)}/s{si}"
            level_kernels(out, tag, mg, 0, dims, omega)
            stencil_table(tag, mg, fine, dims, scaled, omega)
            if si == 0:  # the transfers know nothing of the smoother
                grid_transfers(out, key(dims), mg, 1, fine, dims)
            mg.destroy()


def hierarchies(out):
    grid, levels = M.THREE_LEVEL
    d1, d0 = M.st27_levels(grid, levels, True)
    mg = _mgmc(grid, levels, True, 1.3)
    level_kernels(out, "three/" + key(d1), mg, 1, d1, 1.3)
    level_kernels(out, "three/" + key(d0), mg, 0, d0, 1.3)
    st27_transfers(out, "three/st27", mg, 1, d1, d0)
    grid_transfers(out, "three/grid", mg, 2, grid, d1)
    mg.destroy()
    grid, levels = M.SEMICOARSENED
    (d0,) = M.st27_levels(grid, levels, True)
    mg = _mgmc(grid, levels, False, 1.0)
    level_kernels(out, "semi/" + key(d0), mg, 0, d0, 1.0)
    grid_transfers(out, "semi/grid", mg, 1, grid, d0)
    mg.destroy()
    grid, levels = M.FLAT_QUAD
    mg = _mgmc(grid, levels, False, 1.0)
    grid_transfers(out, "quad/grid", mg, 1, grid, M.coarsen(grid), fused=False)
    mg.destroy()


def vcycle_chain(grid, levels, setting, guesszero):
    """samples of one chain, concatenated; the parent compares them with oracle_chain"""
    from parmgmc_amd import MGMC
    from test_gpu_vcycle_shapes_oracle import SETTINGS

    scaled, omega, sweep, nu, coarse, cits, literal = SETTINGS[setting]
    b, y0 = vcycle_inputs(grid)
    mg = MGMC(*grid, KAPPA, levels)
    mg.set_smoother(scaled, omega, sweep, nu)
    mg.set_coarse(coarse, cits)
    mg.set_correction_form(literal)
    mg.setup()
    seen = []
    y = _dev(np.zeros_like(y0) if guesszero else y0)
    nxt = mg.sample(_dev(b), y, VCYCLE_ITS, seed=VCYCLE_SEED, counter0=VCYCLE_COUNTER0, guesszero=guesszero, callback=lambda it, yy: seen.append(_host(yy)))
    need(nxt == VCYCLE_COUNTER0 + VCYCLE_ITS and np.array_equal(seen[-1], _host(y)), f"vcycle {grid} {setting}: counter or last sample")
    mg.destroy()
    return np.concatenate(seen)


def vcycles(out):
    from test_gpu_vcycle_shapes_oracle import SETTINGS

    for grid, levels in M.VCYCLE_SHAPES.items():
        for setting in SETTINGS:
            out[f"vcycle/{key(grid)}/{setting}"] = vcycle_chain(grid, levels, setting, False)
        out[f"vcycle/{key(grid)}/guesszero"] = vcycle_chain(grid, levels, "default", True)


def main(path):
    import torch

    out = {}
    tabled_shapes(out)
    hierarchies(out)
    vcycles(out)
    torch.cuda.synchronize()
    np.savez(path, **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
