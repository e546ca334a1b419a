"""tests/rbstats_cases.py on the CPU: the case matrices hold what they are there for, the extended-precision reference of the
conditional means satisfies the identity that defines them, and the estimator does what it is built for -- on exact samples and
on the oracle's restatement of the MGMC run of tests/test_gpu_rbstats.py."""
import numpy as np
import pytest

import oracle as O
import rbstats_cases as R

LD_EPS = float(np.finfo(np.longdouble).eps)


@pytest.mark.parametrize("M", [R.random_spd(65, 65), R.random_spd(257, 257)] + R.integer_matrices(), ids=lambda M: M.name)
def test_case_matrices_hold_their_rows(M):
    rows = [list(zip(M.colidx[M.rowptr[i] : M.rowptr[i + 1]], M.vals[M.rowptr[i] : M.rowptr[i + 1]])) for i in range(M.n)]
    assert [c for c, _ in rows[3]] == [3]  # no off-diagonal entry
    assert len(rows[7]) == R.WIDE > 64 and [c for c, _ in rows[7]].count(7) == 1
    cols11 = [int(c) for c, _ in rows[11]]
    assert cols11[-1] == 11 and cols11[:-1] == sorted(cols11[:-1], reverse=True) and len(cols11) > 2  # unsorted, diagonal last
    Q = R.dense(M).astype(np.float64)
    assert np.array_equal(Q, Q.T) and np.linalg.eigvalsh(Q).min() > 0
    assert M.n % 64 != 0 and M.n % 8 != 0  # not a multiple of the rows per wavefront of any split but lpr = 64
    if M.name.endswith("i"):
        assert np.array_equal(M.vals, np.round(M.vals))
        d = R.cond_precision_host(M)
        assert np.array_equal(np.log2(d), np.round(np.log2(d)))


def test_case_table_covers_the_lane_splits():
    from chainstats_cases import lpr_log2_of

    assert {lpr_log2_of(C) for C in R.CHAINS} == set(range(7))
    assert 64 in R.CHAINS and 65 in R.CHAINS and any(C > 64 and C % 64 not in (0, 1) for C in R.CHAINS)  # chunk boundary, partial last chunk
    assert any((1 << lpr_log2_of(C)) != C and C < 64 for C in R.CHAINS)  # a partial lane group
    assert R.MORE_CHAINS == [4, 16, 32, 63, 128, 129] and not set(R.MORE_CHAINS) & set(R.CHAINS)
    assert [lpr_log2_of(C) for C in R.MORE_CHAINS] == [2, 4, 5, 6, 6, 6]  # full lane groups; one dead lane; 2 and 3 chunks
    assert R.RANKS[:3] == [0, 1, 3] and R.RANKS[3] > 3
    for n in (65, 257):
        B, S = R.lowrank(n, 3, seed=n)
        assert not B[n // 2].any() and B[3].all() and (S > 0).all()


@pytest.mark.parametrize("M", R.matrices(), ids=lambda M: M.name)
@pytest.mark.parametrize("k", R.RANKS)
def test_reference_satisfies_the_defining_identity(M, k):
    """m == y + (b - Q y) / diag(Q) with Q assembled densely in extended precision, to bound_m plus what the two sides differ by
    by construction: the float64 host q against the extended-precision diag(Q) (2 k + 1 roundings, relative to |m|) and the
    extended-precision rounding of the dense product"""
    C_ = 5
    Y = R.samples(M.n, C_, seed=M.n + k)
    b = R.rhs(M.n, seed=k)
    lr = R.lowrank(M.n, k, seed=M.n)
    m, bound = R.cond_mean_ref(M, Y, b, lr)
    Q = R.dense(M, lr)
    Yl = Y.astype(np.longdouble)
    d = np.diag(Q)[:, None]
    ident = Yl + (b.astype(np.longdouble)[:, None] - Q @ Yl) / d
    slack = R.gamma(2 * k + 1) * np.abs(m) + 16 * (M.n + 4) * LD_EPS * (np.abs(Yl) + (np.abs(b)[:, None] + np.abs(Q) @ np.abs(Yl)) / d)
    assert (np.abs(m - ident) <= bound + slack).all()
    assert float(np.abs(m - ident).max()) < 1e-14 * float(np.abs(ident).max() + 1)
    assert (bound >= 0).all() and float(bound.max()) < 1e-12
    # the isolated row of the random matrices without a low-rank term: b / q, whatever y is
    if k == 0 and M.name.startswith("spd"):
        assert np.array_equal(m[3], np.broadcast_to(np.longdouble(b[3]) / np.longdouble(R.cond_precision_host(M)[3]), (C_,)))


@pytest.mark.parametrize("dyadic", [True, False])
def test_diagonal_matrix_gives_b_over_q(dyadic):
    M = R.diagonal(67, seed=2, dyadic=dyadic)
    b = R.rhs(67, seed=2, integer=dyadic)
    q = R.cond_precision_host(M)
    m, bound = R.cond_mean_ref(M, R.samples(67, 9, seed=1), b)
    assert np.array_equal(m, np.broadcast_to((b.astype(np.longdouble) / q.astype(np.longdouble))[:, None], m.shape))
    if dyadic:  # exact in float64, and C b / q is exact for every C of the table: the device mean is b / q bit for bit
        assert np.array_equal(m.astype(np.float64).astype(np.longdouble), m)
        for C_ in R.CHAINS + R.MORE_CHAINS:
            assert np.array_equal((C_ * (b / q)) / C_, b / q)


@pytest.mark.parametrize("count,seed", [(64, 0), (64, 1), (400, 0), (1600, 0)])
def test_rao_blackwellised_variance_beats_plain_moments_on_exact_samples(count, seed):
    """exact iid samples L^-T z of N(0, Q^-1) on ex6_matrix(9, 0.05): the relative 2-norm error of the variance field against
    diag(Q^-1) is smaller with 1 / Q_ii + var(m) than with var(y).
    Observed: 64 samples 0.1777 / 0.1349 and 0.1811 / 0.1102 (plain / Rao-Blackwellised), 400: 0.0694 / 0.0394, 1600: 0.0338 / 0.0224."""
    A = O.ex6_matrix(9, 0.05)
    Q = A.scipy().toarray()
    L = np.linalg.cholesky(Q)
    X = np.linalg.solve(L.T, np.random.default_rng(seed).standard_normal((A.n, count))).T
    b = np.ones(A.n)
    mp, mr, vp, vr = R.plain_and_rb_errors(Q, b, X + np.linalg.solve(Q, b)[None, :])
    print(f"{count} samples, seed {seed}: variance error plain {vp:.4f}, Rao-Blackwellised {vr:.4f}")
    assert vr < vp, (vr, vp)
    assert abs(float(np.mean((1 / np.diag(Q)) / np.diag(np.linalg.inv(Q)))) - 0.35) < 0.01  # the exact share of the variance


def test_end_to_end_configuration_on_the_oracle_chain():
    """the configuration of the GPU end-to-end test, evaluated on the oracle's restatement of the same chains: both error ratios
    are at or below 0.9, so that the device chain's 1e-11 parity with the oracle cannot turn err_rb <= err_plain.
    Observed: mean err_plain 0.03060, err_rb 0.02646 (ratio 0.865); variance err_plain 0.07981, err_rb 0.06119 (ratio 0.767)."""
    E = R.E2E
    A, _, _, b = R.e2e_problem()
    chains = R.e2e_oracle_chains(E["burn_in"] + E["window"])
    X = chains[E["burn_in"] :].reshape(-1, A.n)
    assert X.shape == (E["window"] * E["nchains"], A.n)
    mp, mr, vp, vr = R.plain_and_rb_errors(A.scipy().toarray(), b, X)
    print(f"oracle chain: mean err_plain {mp:.5f} err_rb {mr:.5f} ratio {mr / mp:.3f}; variance err_plain {vp:.5f} err_rb {vr:.5f} ratio {vr / vp:.3f}")
    assert mr / mp <= 0.9 and vr / vp <= 0.9
