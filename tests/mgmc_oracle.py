"""The oracle's restatement of the geometric Multigrid Monte Carlo chain (reference src/pc_gamgmc.c:227-264 + PCMG) with
the library's noise streams: shared by the direct-handle tests (test_gpu_mgmc.py) and the PC-layer option tests."""
import numpy as np

import oracle as O

GOLD = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1


def level_seed(seed, l):
    return (seed + GOLD * (l + 1)) & M64


def oracle_hierarchy(nx, ny, nz, kappa, levels):
    dims = [(nx, ny, nz)]
    for _ in range(levels - 1):
        dims.append(tuple((d - 1) // 2 + 1 if d > 1 else 1 for d in dims[-1]))
    dims = dims[::-1]  # dims[0] coarsest
    A = O.shifted_laplace(nx, ny, nz, kappa).scipy()
    lv = [None] * levels
    lv[levels - 1] = dict(A=A, P=None, dims=dims[-1])
    for l in range(levels - 1, 0, -1):
        P = O.q1_interp(*dims[l - 1])
        lv[l]["P"] = P
        lv[l - 1] = dict(A=O.galerkin(lv[l]["A"], P), P=None, dims=dims[l - 1])
    return lv


def oracle_chain(grid, kappa, levels, b, y0, its, seed, counter0, guesszero, nu=1, scaled=False, omega=1.0, sweep=O.SOR_FORWARD, coarse="cholsampler", coarse_its=1, lv=None, shift=None):
    """`lv`: a hierarchy from oracle_hierarchy(grid, kappa, levels) to reuse; `shift`: {level: k} moves that level's noise
    counters by k draws (a negative control: the chain must then differ from the sampler's)"""
    if lv is None:
        lv = oracle_hierarchy(*grid, kappa, levels)
    shift = shift or {}
    top = levels - 1
    csr = [O.CSR.from_scipy(x["A"]) for x in lv]
    cols = [O.coloring_parity8(*x["dims"]) for x in lv]
    cols[top] = O.coloring_redblack(*grid)
    Lc = O.potrf_lower(csr[0].dense()) if coarse == "cholsampler" else None
    y = np.array(y0, copy=True)
    out = []
    for it in range(its):
        s = counter0 + it
        ctr = {l: 64 * s + shift.get(l, 0) for l in range(levels)}

        def noise(l):
            c = ctr[l]
            ctr[l] += 1
            if l == top:
                return O.noise_grid(*grid, level_seed(seed, l), c)
            return O.noise_rows(csr[l].n, level_seed(seed, l), c)

        def smooth(l, rhs, x, leg, its_=None):
            return O.gibbs_samples(csr[l], cols[l], rhs, x, nu if its_ is None else its_, lambda d: noise(l), omega, sweep, scaled)

        def coarse_fn(rhs):
            if coarse == "cholsampler":
                return O.chol_sample(Lc, rhs, noise(0))
            return smooth(0, rhs, np.zeros(csr[0].n), 0, coarse_its)

        y = O.gamgmc_richardson(lv, b, y, 1, guesszero and it == 0, smooth, coarse_fn)
        out.append(y.copy())
    return out


class LrcMgmcOracle:
    """The oracle's restatement of PCGAMGMC on a MATLRC operator: the hierarchy of the base matrix, per-level
    factors B_l, level samplers = LRC Gibbs sweeps (src/mc_sor.c:101-112, src/pc_mcgibbs.c:130-140), level residuals
    with the LRC operator (src/pc_gamgmc.c:186-194), coarse = Cholesky of the explicit sum (src/pc_chols.c:119-153)."""

    def __init__(self, lv, colors, B, S, nu=1, omega=1.0, sweep=O.SOR_FORWARD, scaled=True, coarse="cholsampler", coarse_its=1):
        self.base, self.colors, self.S = lv, colors, np.asarray(S, float)
        self.nu, self.omega, self.sweep, self.scaled, self.coarse, self.coarse_its = nu, omega, sweep, scaled, coarse, coarse_its
        self.Bl = O.lrc_level_factors(lv, B)
        self.csr = [O.CSR.from_scipy(x["A"]) for x in lv]
        self.lv = [dict(A=O.LRCOperator(x["A"], self.Bl[l], self.S), P=x["P"]) for l, x in enumerate(lv)]
        dirs = [O.SOR_FORWARD, O.SOR_BACKWARD]
        self.Bb = [{d: O.lrc_build_correction(self.csr[l], colors[l], self.Bl[l], self.S, omega, d) for d in dirs} for l in range(len(lv))]
        self.sd = [O.sqrtdiag(self.csr[l], omega, scaled) for l in range(len(lv))]
        self.Lc = O.potrf_lower(self.lv[0]["A"].dense()) if coarse == "cholsampler" else None
        self.ndir = 2 if sweep == O.SOR_SYMMETRIC else 1

    def draws_per_smooth(self, l):
        return (self.coarse_its if (l == 0 and self.coarse == "gibbs") else self.nu) * self.ndir

    def sweeps(self, l, rhs, x, its, xi_fn, eta_fn):
        """its samples of the level sampler; xi_fn(d) / eta_fn(d) = the d-th directional sweep's draws"""
        d = 0
        sq = np.sqrt(np.abs(self.S))
        for _ in range(its):
            for direction in ([O.SOR_FORWARD, O.SOR_BACKWARD] if self.sweep == O.SOR_SYMMETRIC else [self.sweep]):
                w = O.prepare_rhs(xi_fn(d), self.sd[l], rhs) + self.Bl[l] @ (sq * eta_fn(d))
                d += 1
                x = O.lrc_mcsor_apply(self.csr[l], self.colors[l], self.Bl[l], self.Bb[l][O.SOR_FORWARD], self.Bb[l][O.SOR_BACKWARD], w, x, self.omega, direction)
        return x

    def chain(self, b, y, its, guesszero, xi, eta, chol_xi):
        """xi(l, c) / eta(l, c): the c-th draw of level l in this chain call (c counts from 0 per SAMPLE via the
        caller's closures); chol_xi(c) the coarse Cholesky draw."""
        top = len(self.lv) - 1
        for it in range(its):
            ctr = {l: 0 for l in range(top + 1)}

            def smooth(l, rhs, x, leg, n=None):
                n = self.nu if n is None else n
                c0 = ctr[l]
                ctr[l] += n * self.ndir
                return self.sweeps(l, rhs, x, n, lambda d: xi(it, l, c0 + d), lambda d: eta(it, l, c0 + d))

            def coarse_fn(rhs):
                if self.coarse == "cholsampler":
                    return O.chol_sample(self.Lc, rhs, chol_xi(it))
                return smooth(0, rhs, np.zeros(len(rhs)), 0, self.coarse_its)

            y = O.gamgmc_richardson(self.lv, b, y, 1, guesszero and it == 0, smooth, coarse_fn)
        return y
