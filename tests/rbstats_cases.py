"""Cases and an extended-precision reference of the Rao-Blackwellised chain statistics (pmg_rbstats_*, kernels_rbstats.hip).
Importable without a device; tests/test_rbstats_cases.py checks this module on the CPU, tests/test_gpu_rbstats.py runs the
library against it.

The estimator: for x ~ N(Q^-1 b, Q^-1) and a sample y, m_i = (b_i - sum_{j != i} Q_ij y_j) / Q_ii is E[x_i | x_-i]; the mean of m
estimates E[x_i] and 1 / Q_ii + the variance of m estimates Var[x_i].  Q = A, or A + B diag(S) B^T.

The arithmetic contract (include/parmgmc_hip.h) per row i and chain c, every operation rounded on its own:
    s = 0.0;  s = s + a_ij * y_jc                                over the stored off-diagonal entries in stored order
    w = 0.0;  w = w + (B_ik * S_k) * (t_kc - B_ik * y_ic)        k ascending, t = B^T y from the chain kernel of the samplers
    m = ((b_i - s) - w) / q_i,   q_i = a_ii + sum_k S_k * (B_ik * B_ik)      (q on the host, k ascending)

FORWARD-ERROR BOUND of m against np.longdouble (bound_m), gamma_p = p eps / (1 - p eps):
  * an off-diagonal term a_ij y_jc passes through its product, at most len - 1 additions of s (the first one, to 0.0, is exact),
    b - s, r - w and the division: at most len + 3 roundings with a low-rank term, len + 2 without; b_i through at most 3.
    Both are covered by gamma_{len + k + 2}, len = stored off-diagonal entries of the row.
  * a low-rank term passes through B S, B y, the difference, the product, at most k - 1 additions of w, r - w and the division:
    at most k + 5 roundings.  That is below len + k + 2 from three off-diagonal entries on; for shorter rows the term is weighted
    by gamma_{k + 5}, without which the expression would not be a bound there.
  * t_kc itself is an n-term sum formed by another kernel: its recursive-summation bound gamma_n sum_j |B_jk| |y_jc| enters
    through |B_ik S_k|.
  * q is the float64 host formula on both sides (tests/test_rbstats_boundary.py pins it bit for bit), so it adds nothing.
    bound_m = (gamma_{len+k+2} (|b_i| + sum_j |a_ij| |y_j|) + gamma_{max(len+k+2, k+5)} L_i + T_i) / q_i,
    L_i = sum_k |B_ik S_k| (|t_k| + |B_ik y_i|),   T_i = sum_k |B_ik S_k| gamma_n sum_j |B_jk| |y_j|.

BOUNDS OF THE FIELDS (fields_reference): the fields are the moments of the m the device forms.  With e = m_device - m_ref,
|e_ic| <= d_i = the largest bound_m of row i over the steps, and N samples per row:
    |mean(m_device) - mean(m_ref)| <= d_i
    |var(m_device) - var(m_ref)| = |2 sum (m - mean)(e - ebar) + sum (e - ebar)^2| / (N - 1)
                                <= 2 sqrt(var(m_ref)) d_i sqrt(N / (N - 1)) + d_i^2 N / (N - 1)            (Cauchy-Schwarz)
on top of the bounds tests/chainstats_cases.longdouble_fields gives for moments formed in the order of kernels_chainstats.hip,
plus two roundings (1 / q and the final sum) of relative size eps each on the variance.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import oracle as O
from chainstats_cases import longdouble_fields

EPS = np.finfo(np.float64).eps
# every lpr (9 and 17 are there for the splits of 16 and 32 lanes per row), a partial last lane group, the chunk boundary, a
# partial last chunk
CHAINS = [1, 2, 3, 5, 8, 9, 17, 33, 64, 65, 130]
# the full lane groups of 4, 16 and 32 lanes per row, one chain short of a full chunk, and the second chunk edge: two full chunks |
# three chunks with a last chunk of one chain
MORE_CHAINS = [4, 16, 32, 63, 128, 129]
RANKS = [0, 1, 3, 5]  # pmg_mcsor_set_lowrank's chain path takes k <= 64: 5 is the rank above 3
WIDE = 70  # stored entries of the wide row: more than one wavefront of lanes at lpr = 1

Matrix = namedtuple("Matrix", "name rowptr colidx vals n why")


def gamma(p):
    return p * EPS / (1 - p * EPS)


def _csr(rows, name, why):
    """rows: one list of (column, value) per row, in the order they are to be stored"""
    rowptr = np.zeros(len(rows) + 1, np.int32)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    colidx = np.array([c for r in rows for c, _ in r], np.int32)
    vals = np.array([v for r in rows for _, v in r], np.float64)
    return Matrix(name, rowptr, colidx, vals, len(rows), why)


def random_spd(n, seed, integer=False):
    """A symmetric, strictly diagonally dominant (so SPD) n x n matrix, n >= 65, that holds
         row 3:  no off-diagonal entry;
         row 7:  WIDE stored entries -- the diagonal and 69 off-diagonal entries; where n - 2 < 69 columns are there to couple
                 to (row 3 stays isolated), the first ones are stored twice, each time with half the value (a CSR may list a
                 column twice: the entries add);
         row 11: columns stored in descending order with the diagonal LAST (the stored-order contract);
       every other row ascending.  integer: off-diagonal entries in {-3 .. 3} \\ {0} (halves of even values where split) and a
       power-of-two diagonal, so that with integer y and b no operation of the contract rounds."""
    rng = np.random.default_rng(seed)
    off = [dict() for _ in range(n)]

    def couple(i, j, v):
        if i != j and 3 not in (i, j) and j not in off[i]:
            off[i][j] = off[j][i] = v

    def value():
        return float(rng.choice([-3, -2, -1, 1, 2, 3])) if integer else float(rng.uniform(-1.0, 1.0))

    for i in range(n):
        for j in rng.choice(n, 3, replace=False):
            couple(i, int(j), value())
    for j in range(n):
        if len(off[7]) == min(WIDE - 1, n - 2):
            break
        if j != 7:
            couple(7, j, value())
    short = (WIDE - 1) - len(off[7])  # columns of row 7 to store twice
    assert 0 <= short <= len(off[7])
    if integer:  # the halves must stay integers
        for j in sorted(off[7])[:short]:
            off[7][j] = off[j][7] = 2.0 * off[7][j]
    rows = []
    for i in range(n):
        dom = sum(abs(v) for v in off[i].values()) + 1.0
        diag = float(2.0 ** np.ceil(np.log2(dom))) if integer else dom + float(rng.uniform(0.0, 1.0))
        ent = sorted(off[i].items())
        if i == 7:
            ent = [(j, v / 2) for j, v in ent[:short]] + ent[short:] + [(j, v / 2) for j, v in ent[:short]]
            assert len(ent) == WIDE - 1
            rows.append(ent[:20] + [(i, diag)] + ent[20:])
        elif i == 11:
            rows.append(ent[::-1] + [(i, diag)])
        else:
            rows.append(sorted(ent + [(i, diag)]))
    return _csr(rows, f"spd{n}" + ("i" if integer else ""), f"{n} rows: an isolated row, a row of {WIDE} entries, a row stored backwards with the diagonal last")


def ex6():
    A = O.ex6_matrix(9, 0.05)
    return Matrix("ex6", A.rowptr, A.colidx, A.vals, A.n, "ex6_matrix(9, 0.05): the operator of DESIGN 11.2 and 12, 81 rows")


def one_row():
    return _csr([[(0, 2.5)]], "one", "n = 1: one live lane group, three idle wavefronts")


def diagonal(n, seed, dyadic=False):
    """dyadic: power-of-two entries, so that b / q with integer b has few bits and C b / q is exact for every C of the table"""
    rng = np.random.default_rng(seed)
    d = 2.0 ** rng.integers(-2, 4, n) if dyadic else rng.uniform(0.5, 4.0, n)
    return _csr([[(i, float(d[i]))] for i in range(n)], f"diag{n}", "a diagonal Q: m = b / q whatever y is")


def matrices():
    return [ex6(), one_row(), random_spd(65, 65), random_spd(257, 257)]


def integer_matrices():
    return [random_spd(65, 165, integer=True), random_spd(257, 1257, integer=True)]


def lowrank(n, k, seed):
    """(B, S) or None for k = 0: B (n, k) dense with row n // 2 zero (and row 3, the isolated row, when it exists, nonzero), S > 0"""
    if k == 0:
        return None
    rng = np.random.default_rng(1000 * k + seed)
    B = rng.uniform(-1.0, 1.0, (n, k)) / np.sqrt(n)
    B[n // 2] = 0.0
    return np.asfortranarray(B), rng.uniform(0.5, 20.0, k)


def samples(n, C, seed, integer=False):
    rng = np.random.default_rng(seed)
    if integer:
        return rng.integers(-8, 9, (n, C)).astype(np.float64)
    return rng.standard_normal((n, C)) * rng.uniform(0.1, 3.0, (n, 1)) + 0.5


def rhs(n, seed, integer=False):
    rng = np.random.default_rng(seed + 17)
    return rng.integers(-8, 9, n).astype(np.float64) if integer else rng.standard_normal(n)


def dense(M, lr=None):
    """Q as a dense longdouble matrix (stored entries of one position add)"""
    Q = np.zeros((M.n, M.n), np.longdouble)
    for i in range(M.n):
        for j in range(M.rowptr[i], M.rowptr[i + 1]):
            Q[i, M.colidx[j]] += np.longdouble(M.vals[j])
    if lr is not None:
        B, S = lr
        Bl = B.astype(np.longdouble)
        Q += (Bl * S.astype(np.longdouble)) @ Bl.T
    return Q


def cond_precision_host(M, lr=None):
    """q_i = a_ii + sum_k S_k * (B_ik * B_ik), k ascending, one float64 rounding per operation: the host formula of the header"""
    q = np.empty(M.n)
    for i in range(M.n):
        d = [M.vals[j] for j in range(M.rowptr[i], M.rowptr[i + 1]) if M.colidx[j] == i]
        assert len(d) == 1
        q[i] = d[0]
    if lr is not None:
        B, S = lr
        for k in range(len(S)):
            q = q + S[k] * (B[:, k] * B[:, k])
    return q


def cond_mean_ref(M, Y, b=None, lr=None):
    """(m, bound): np.longdouble conditional means of Y (n, C) with the float64 host q, and bound_m of the module docstring"""
    n, C = Y.shape
    assert n == M.n
    q = cond_precision_host(M, lr).astype(np.longdouble)
    Yl = Y.astype(np.longdouble)
    bl = np.zeros(n, np.longdouble) if b is None else b.astype(np.longdouble)
    s = np.zeros((n, C), np.longdouble)
    sabs = np.zeros((n, C), np.longdouble)
    length = np.zeros(n, np.int64)
    for i in range(n):
        for j in range(M.rowptr[i], M.rowptr[i + 1]):
            c = M.colidx[j]
            if c != i:
                a = np.longdouble(M.vals[j])
                s[i] += a * Yl[c]
                sabs[i] += abs(a) * np.abs(Yl[c])
                length[i] += 1
    k = 0 if lr is None else len(lr[1])
    w = np.zeros((n, C), np.longdouble)
    L = np.zeros((n, C), np.longdouble)
    T = np.zeros((n, C), np.longdouble)
    if lr is not None:
        Bl, Sl = lr[0].astype(np.longdouble), lr[1].astype(np.longdouble)
        t = Bl.T @ Yl  # k x C
        tabs = np.abs(Bl).T @ np.abs(Yl)
        for kk in range(k):
            bs = (Bl[:, kk] * Sl[kk])[:, None]
            by = Bl[:, kk][:, None] * Yl
            w += bs * (t[kk][None, :] - by)
            L += np.abs(bs) * (np.abs(t[kk])[None, :] + np.abs(by))
            T += np.abs(bs) * (gamma(n) * tabs[kk])[None, :]
    m = ((bl[:, None] - s) - w) / q[:, None]
    p = length + k + 2
    g_main = np.array([gamma(int(x)) for x in p], np.longdouble)[:, None]
    g_lr = np.array([gamma(int(max(x, k + 5))) for x in p], np.longdouble)[:, None]
    bound = (g_main * (np.abs(bl)[:, None] + sabs) + g_lr * L + T) / q[:, None]
    return m, bound


def fields_reference(m_steps, bound_steps, q):
    """(mean_ref, var_ref, mean_bound, var_bound) of the fields after the steps whose longdouble conditional means and bounds
    (cond_mean_ref) are given; q = cond_precision_host.  The bounds are those of the module docstring, per row."""
    T, (_, C) = len(m_steps), m_steps[0].shape
    N = T * C
    m_ref, v_ref, mean_b, var_b = longdouble_fields(m_steps)
    d = np.max(np.concatenate(bound_steps, axis=1), axis=1)
    ql = q.astype(np.longdouble)
    var_ref = 1 / ql + v_ref
    mean_bound = mean_b + d
    var_bound = var_b + 2 * np.sqrt(v_ref) * d * np.sqrt(N / (N - 1.0)) + d * d * (N / (N - 1.0)) + EPS * (1 / ql) + EPS * var_ref
    return m_ref, var_ref, mean_bound, var_bound


def rel2(x, ref):
    """relative 2-norm error"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


def plain_and_rb_errors(Q, b, samples_):
    """relative 2-norm errors (mean_plain, mean_rb, var_plain, var_rb) of the two estimators on `samples_` (N, n) of
    N(Q^-1 b, Q^-1) against Q^-1 b and diag(Q^-1): float64 numpy, for the statistical comparisons"""
    Q = np.asarray(Q, np.float64)
    Sigma = np.linalg.inv(Q)
    mu = Sigma @ b
    q = np.diag(Q)
    X = np.asarray(samples_, np.float64)
    M = X + (b[None, :] - X @ Q.T) / q[None, :]
    return (rel2(X.mean(axis=0), mu), rel2(M.mean(axis=0), mu), rel2(X.var(axis=0, ddof=1), np.diag(Sigma)), rel2(1 / q + M.var(axis=0, ddof=1), np.diag(Sigma)))


# ---- the end-to-end comparison of tests/test_gpu_rbstats.py --------------------------------------------------------------------
# 8 chains of MGMC (forward Gibbs, nu = 1, exact coarse sampler) on the ~1000-row ex6 operator of tests/test_gpu_chainstats.py from
# Y = 0, its burn-in of 50 steps, then `window` recorded steps.  Seeds and window were fixed on the CPU from the oracle's chain
# (e2e_oracle_chains): err_rb / err_plain = 0.865 for the mean and 0.767 for the variance there.  Of the 24 (seed base, window)
# pairs scanned -- bases 0xE7, 0xCAFE, 0x51, windows 10 .. 200 -- the variance ratio was 0.73 .. 0.82 everywhere; the mean ratio
# was 0.865 .. 0.95, at or below 0.9 for 4 of them: on this sampler the gain on the mean is small, and the ratios do not depend
# on b (the chain is linear in it).
E2E = dict(n=32, kappa=1e-2, coarse_max=100, nchains=8, burn_in=50, window=50, seeds=[0xCAFE + 7919 * c for c in range(8)], rhs_seed=6)


def e2e_problem():
    """(A, ops, ps, b): the operator, its aggregation hierarchy (parmgmc_amd.unstructured.build_hierarchy) and the right-hand side"""
    from parmgmc_amd.unstructured import build_hierarchy

    A = O.ex6_matrix(E2E["n"], E2E["kappa"])
    ops, ps = build_hierarchy(A.scipy().tocsr(), coarse_max=E2E["coarse_max"])
    return A, ops, ps, np.random.default_rng(E2E["rhs_seed"]).standard_normal(A.n)


def e2e_oracle_chains(steps):
    """(steps, nchains, n): the oracle's restatement of the chains MGMC.sample_chains(b, Y = 0, steps, seeds) runs on e2e_problem()
    -- greedy colouring on every level, row-stream noise with 64 counters per sample, as tests/test_gpu_mgmc.py restates it"""
    import scipy.sparse as sp
    from mgmc_oracle import level_seed

    A, ops, ps, b = e2e_problem()
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
