"""tests/woodbury_cases.py without a GPU: the chain counts reach every lane split of kernels_lrc_chains.hip and
kernels_chains.hip, the restated constants are the kernels', the case table covers what it says, the plain float64
evaluation of every case passes every bound, a dropped row or a wrong last entry of S does not, and the extended-precision
reference agrees with a 40-digit evaluation."""
import re
from pathlib import Path

import numpy as np
import pytest

import woodbury_cases as W

CSRC = Path(__file__).resolve().parent.parent / "parmgmc_amd" / "csrc"
IDS = [W.case_id(c) for c in W.CASES]


def test_chain_counts_reach_every_lane_split():
    counts = W.CHAINS + W.CONTROLS
    assert sorted(counts) == sorted(W.CHAIN_TABLE) and len(set(counts)) == len(counts)
    for C, row in W.CHAIN_TABLE.items():
        assert row == W.lane_split(C), C
    lprl = lambda C: W.CHAIN_TABLE[C][0]  # noqa: E731
    assert {lprl(C) for C in counts} == set(range(7))
    # what the suite ran before (the controls) left LPRL 1 and 4 out
    assert {lprl(C) for C in W.CONTROLS} == {0, 2, 3, 5, 6} and {lprl(C) for C in W.CHAINS} >= {1, 4}
    # every power of two up to 64 itself (every lane of a group live) and a count behind it, in the next lane split
    for p in (1, 2, 4, 8, 16, 32):
        assert p in counts and lprl(p) == p.bit_length() - 1
        assert any(p < C <= 2 * p and lprl(C) == lprl(p) + 1 for C in counts), p
    # right behind a power of two: a lane group with all but one of its upper half dead
    assert {3, 9, 17, 33, 65, 129} <= set(counts)
    # one chunk with dead lanes, one chunk full, the chunk edges 64 | 65 and 128 | 129
    assert W.CHAIN_TABLE[33][1:] == (1, 33) and W.CHAIN_TABLE[63][1:] == (1, 63) and W.CHAIN_TABLE[64][1:] == (1, 64)
    assert W.CHAIN_TABLE[65][1:] == (2, 1) and W.CHAIN_TABLE[128][1:] == (2, 64) and W.CHAIN_TABLE[129][1:] == (3, 1)
    assert set(W.CHAIN_WRAP_COUNTS) <= set(counts) and {lprl(C) for C in W.CHAIN_WRAP_COUNTS} == {1, 4, 6}


def test_restated_constants_are_the_kernels():
    lrc = (CSRC / "kernels_lrc.hip").read_text()
    chains = (CSRC / "kernels_lrc_chains.hip").read_text()
    plain = (CSRC / "kernels_chains.hip").read_text()
    # dense B^T y: blocks of 4096 rows, 256 threads, 16 fma per thread
    assert f"r0 = (int64_t)blockIdx.x * {W.DENSE_ROWS_PER_BLOCK};" in lrc and f"r < r0 + {W.DENSE_ROWS_PER_BLOCK} && r < n; r += 256" in lrc
    assert f"return (int)((n + {W.DENSE_ROWS_PER_BLOCK - 1}) / {W.DENSE_ROWS_PER_BLOCK});" in lrc
    assert "launch_btx<16, false>" in chains and 256 * 16 == W.DENSE_ROWS_PER_BLOCK
    # compact form: 256 * PMG_LRC_RPT rows
    rpt = int(re.search(r"#define PMG_LRC_RPT (\d+)", lrc).group(1))
    assert 256 * rpt == W.COMPACT_ROWS_PER_BLOCK and "return 256 * PMG_LRC_RPT;" in lrc
    assert "launch_btx<4, true>" in chains and "btx_block<4, true, LPRL>" in chains and "ns > 256 * 4" in chains
    assert int(re.search(r"constexpr int KB\s*=\s*(\d+);", chains).group(1)) == W.KB
    # the reduction: 64 lanes, lane l adds the blocks l, l + 64, ...
    assert f"for (int b = lane; b < nblocks; b += {W.REDUCE_LANES})" in lrc and "__launch_bounds__(64) void lrc_reduce_kernel" in lrc
    assert f"for (int b = l; b < nb; b += {W.REDUCE_LANES})" in chains and "tree_node<64>(0, leaf, v);" in chains
    # the lane split: the count rounded up to a power of two, at most 64 lanes; chunks of 64 chains
    assert "while (l < 6 && (1 << l) < C) ++l;" in chains and "return (unsigned)((C + 63) / 64);" in chains
    assert "if (C >= 64) m.lpr_log2 = 6;" in plain and "while ((1 << m.lpr_log2) < C) ++m.lpr_log2;" in plain
    # one instantiation per lane split, dense, compact and one-block
    for l in range(6):
        assert f"case {l}: hipLaunchKernelGGL((lrc_btx_chains_kernel<R, ROWS, {l}>)" in chains
        assert f"case {l}: hipLaunchKernelGGL((lrc_small_chains_kernel<{l}>)" in chains
    assert "default: hipLaunchKernelGGL((lrc_btx_chains_kernel<R, ROWS, 6>)" in chains and "default: hipLaunchKernelGGL((lrc_small_chains_kernel<6>)" in chains
    # the depth of B^T y's sums stays under the bound's 64 for every tabled n
    for c in W.CASES:
        nb = -(-c.n // W.DENSE_ROWS_PER_BLOCK)
        assert 16 + 6 + 2 + -(-nb // W.REDUCE_LANES) + 6 <= W.BTX_DEPTH


def test_case_table_covers_what_it_says():
    cases = W.CASES
    assert len(set(cases)) == len(cases)
    assert {c.n for c in cases} == set(W.NS) | {W.N_WRAP} and {c.k for c in cases} == set(W.KS)
    for k in W.KS:
        assert sum(c.k == k for c in cases) >= 2, k
    # k on both sides of KB and of 2 KB, an odd one, and the LDS arrays' 64
    assert {W.KB, W.KB + 1, 2 * W.KB, 2 * W.KB + 1, 64} <= set(W.KS) and any(k < W.KB for k in W.KS) and any(k % 2 for k in W.KS if k > 1)
    assert W.Case(8193, 64, False, False, False) in cases and W.Case(8193, 64, True, True, False) in cases
    # one row, one block less a row, one block, one block and a row, two blocks and a row; 65 blocks: the reduce lanes wrap
    B = W.DENSE_ROWS_PER_BLOCK
    assert {B - 1, B, B + 1, 2 * B + 1} <= set(W.NS) and -(-W.N_WRAP // B) == W.REDUCE_LANES + 1
    assert sorted(c.k for c in cases if c.n == W.N_WRAP) == [5, 9]
    for flag in ("mixed", "perm", "pad"):
        assert any(getattr(c, flag) and c.n <= B for c in cases) and any(getattr(c, flag) and c.n > B for c in cases), flag
    for n, k in W.CHAIN_SHAPES + [W.CHAIN_WRAP_SHAPE]:
        assert W.chain_case(n, k).n == n and k in W.KS
    assert {n for n, _ in W.CHAIN_SHAPES} == {257, 4097} and {k for _, k in W.CHAIN_SHAPES} == {1, 4, 5, 64}


def test_inputs_follow_the_recipe():
    c = W.Case(4097, 4, True, False, True)
    I = W.inputs(c)
    assert I.ldb == c.n + 3 and I.B_host.shape == (c.n + 3, c.k) and I.B_host.flags.f_contiguous
    assert np.isnan(I.B_host[c.n:]).all() and np.array_equal(I.B_host[: c.n], I.B)
    assert ((I.B != 0).sum(0) == c.n // 3).all() and (I.B < 0).any() and (I.B > 0).any()
    assert (I.S[1::2] < 0).all() and (I.S[0::2] > 0).all() and ((np.abs(I.S) >= 20) & (np.abs(I.S) <= 90)).all()
    nz = np.abs(I.B[I.B != 0]) * np.sqrt(c.n // 3)
    assert nz.min() >= 0.5 and nz.max() <= 1.5
    P = W.inputs(W.Case(63, 5, False, True, False))
    d = P.B[:, 0][P.B[:, 0] != 0] / P.C[:, 1][P.B[:, 0] != 0]  # column j of B / d sits in column j + 1 of C
    assert d.min() >= 2 and d.max() <= 6
    T = np.asarray(W.reference(W.Case(63, 5, False, True, False)).T, np.float64)
    assert not np.allclose(T, T.T) and (np.abs(T).argmax(0) != np.arange(5)).all()  # the inverse has to pivot in every column
    one = W.inputs(W.Case(1, 1, False, False, False))
    assert one.B.shape == (1, 1) and 0.5 <= one.B[0, 0] <= 1.5
    for s in W.noise_key(c) + tuple(W.chain_seeds(129)):
        assert s >> 32 and s & 0xFFFFFFFF and s <= W.MASK64  # full 64-bit values
    assert W.chain_seeds(129)[:17] == W.chain_seeds(17) and len(set(W.chain_seeds(129))) == 129


def test_g_margin_is_four_times_the_largest_measured_ratio():
    assert list(W.G_RATIOS_MEASURED) == IDS
    worst = max(W.G_RATIOS_MEASURED.values())
    assert W.G_MARGIN == 2.0 ** np.ceil(np.log2(4.0 * worst)) and W.G_MARGIN <= 64.0


def test_extended_precision_is_extended():
    assert np.finfo(W.L).eps < 2e-19


@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_float64_evaluation_passes_and_the_wrong_ones_fail(case):
    I, R = W.inputs(case), W.reference(case)
    assert 1.0 <= R.cond <= W.COND_CAP
    seed, counter = W.noise_key(case)
    E = W.float64_evaluation(I, seed, counter)
    assert W.g_ratio(E.G, R) <= W.G_MARGIN
    w, wb = W.noisy_rhs_ref(R, I.b, seed, counter)
    assert W.excess(E.w, w, wb) <= 1.0
    y1, yb = W.correct_ref(R, I.y)
    assert W.excess(E.y, y1, yb) <= 1.0
    y1g, ybg = W.correct_ref(R, I.y, G=E.G)
    assert W.excess(E.y, y1g, ybg) <= 1.0
    t, dt = W.btx_ref(R, I.y)
    assert W.excess(I.B.T @ I.y, t, dt) <= 1.0
    # one row left out of B^T y
    r = W.heaviest_row(R, I.y)
    D = W.float64_evaluation(I, seed, counter, drop_row=r)
    assert W.excess(D.y, y1, yb) > 1e3 and W.excess(D.y, y1g, ybg) > 1e3
    yd, ybd = W.correct_ref(R, I.y, drop_row=r)
    assert W.excess(E.y, yd, ybd) > 1e3
    # the last entry of S doubled
    S2 = I.S.copy()
    S2[-1] *= 2.0
    F = W.float64_evaluation(I, seed, counter, S=S2)
    assert W.excess(F.w, w, wb) > 1e3 and W.g_ratio(F.G, R) > 1e3 * W.G_MARGIN
    R2 = W.build(I.B, I.C, S2)
    w2, wb2 = W.noisy_rhs_ref(R2, I.b, seed, counter)
    assert W.excess(E.w, w2, wb2) > 1e3 and W.g_ratio(E.G, R2) > 1e3 * W.G_MARGIN
    # a NaN anywhere is outside every bound
    bad = E.w.copy()
    bad[-1] = np.nan
    assert W.excess(bad, w, wb) == float("inf")


def test_reference_agrees_with_forty_digits():
    import mpmath as mp

    case = W.Case(63, 5, False, True, False)
    I, R = W.inputs(case), W.reference(case)
    seed, counter = W.noise_key(case)
    with mp.workdps(40):
        M = lambda a: mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(a)])  # noqa: E731
        B, Cm = M(I.B), M(I.C)
        T = B.T * Cm
        for j in range(case.k):
            T[j, j] += 1 / mp.mpf(float(I.S[j]))
        G = Cm * mp.inverse(T)
        xi = W.O.noise_rows(case.k, seed, counter)
        c = mp.matrix([mp.sqrt(abs(mp.mpf(float(s)))) * mp.mpf(float(x)) for s, x in zip(I.S, xi)])
        w = M(I.b).T + B * c
        y = M(I.y).T
        t = B.T * y
        y1 = y - G * t
        # 1e-3 of the bounds and of the floor of G: the reference's own error does not count in them
        back = lambda m: np.array([[W.L(mp.nstr(m[i, j], 30)) for j in range(m.cols)] for i in range(m.rows)])  # noqa: E731
        w_ref, wb = W.noisy_rhs_ref(R, I.b, seed, counter)
        y_ref, yb = W.correct_ref(R, I.y)
        t_ref, dt = W.btx_ref(R, I.y)
        assert (np.abs(back(w)[:, 0] - w_ref) <= 1e-3 * wb).all()
        assert (np.abs(back(y1)[:, 0] - y_ref) <= 1e-3 * yb).all()
        assert (np.abs(back(t)[:, 0] - t_ref) <= 1e-3 * dt).all()
        assert np.abs(back(G) - R.G).max() <= 1e-3 * W.g_floor(R)
        assert np.abs(back(T) - R.T).max() <= 1e-18 * float(np.abs(R.T).max())
