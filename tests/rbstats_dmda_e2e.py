"""The end-to-end comparison of the two estimators on a DMDA handle (tests/test_gpu_rbstats_dmda_e2e.py): configuration and the
oracle's restatement of the chain.  Importable without a device; tests/test_rbstats_dmda_e2e.py evaluates it on the CPU.

oracle.ex6_matrix (the operator of DESIGN 11.5's table) is not the DMDA operator: its off-diagonal entries are -1 and its
diagonal is (number of neighbours) + kappa.  The 33 x 33 x 1 DMDA operator with kappa^2 = 0.01 / 32^2 is that matrix at n = 33
times hinv2 = 1 / 32^2 (up to rounding), so the chain has the same correlations and the estimators the same relative errors as
on the table's operator; the sampler is the table's: 8 chains of MGMC on the aggregation hierarchy of the assembled operator
(forward Gibbs, nu = 1, exact coarse sampler) from Y = 0, 50 steps of burn-in, then `window` recorded steps.
Seeds and window were fixed on the CPU from the oracle's chain (oracle_chains): err_rb / err_plain of the variance field is 0.9
or less there (tests/test_rbstats_dmda_e2e.py asserts it and records the figures)."""
import numpy as np

import oracle as O

E2E = dict(grid=(33, 33, 1), kappa=0.1 / 32, coarse_max=100, nchains=8, burn_in=50, window=50, seeds=[0xCAFE + 7919 * c for c in range(8)], rhs_seed=6)


def problem():
    """(A, ops, ps, b): the assembled DMDA operator, its aggregation hierarchy and the right-hand side (the table's b / 32: Q^-1 is 32^2 times that of
    the table's operator, so the samples are 32 times as large and so is the mean with this b)"""
    from parmgmc_amd.unstructured import build_hierarchy

    A = O.shifted_laplace(*E2E["grid"], E2E["kappa"])
    ops, ps = build_hierarchy(A.scipy().tocsr(), coarse_max=E2E["coarse_max"])
    return A, ops, ps, np.random.default_rng(E2E["rhs_seed"]).standard_normal(A.n) / 32


def oracle_chains(steps):
    """(steps, nchains, n): rbstats_cases.e2e_oracle_chains on problem()"""
    import scipy.sparse as sp
    from mgmc_oracle import level_seed

    A, ops, ps, b = problem()
    csr = [O.CSR(*o) for o in ops]
    mats = [c.scipy().tocsr() for c in csr]
    lv = [dict(A=mats[l], P=None if ps[l] is None else sp.csr_matrix((ps[l][2], ps[l][1], ps[l][0]), shape=(csr[l].n, csr[l - 1].n))) for l in range(len(ops))]
    cols = [O.coloring_greedy(c) for c in csr]
    Lc = O.potrf_lower(csr[0].dense())
    out = np.zeros((steps, E2E["nchains"], A.n))
    for c, seed in enumerate(E2E["seeds"]):
        y = np.zeros(A.n)
        for s in range(steps):
            ctr = {l: 64 * s for l in range(len(ops))}

            def noise(l):
                k = ctr[l]
                ctr[l] += 1
                return O.noise_rows(csr[l].n, level_seed(seed, l), k)

            smooth = lambda l, rhs_, x, leg: O.gibbs_samples(csr[l], cols[l], rhs_, x, 1, lambda d: noise(l), 1.0, O.SOR_FORWARD, True)
            y = O.gamgmc_richardson(lv, b, y, 1, False, smooth, lambda rhs_: O.chol_sample(Lc, rhs_, noise(0)))
            out[s, c] = y
    return out
