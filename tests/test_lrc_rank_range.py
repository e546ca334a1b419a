"""The low-rank (MATLRC) update at the top of its rank range, CPU only.

  - The oracle's Woodbury-repaired sweep (O.lrc_mcsor_apply, the restatement of MCSORBuildLRCCorrection + MCSORPostSOR_LRC,
    reference src/mc_sor.c:101-112, :480-544) is checked at k = 64 against a ground truth that does not use its formulas:
    one SOR step on the explicit sum, y_new = (M + B S B^T)^-1 (b + N y) with A = M - N, M = D + L in the sweep's colour
    ordering, solved densely.  test_gpu_lrc_ranks.py holds the device to this oracle at the same ranks.
  - Every entry point that takes a rank and can be called without a device rejects k = -1 and k = 65 with
    PMG_ERR_ARG_OUTOFRANGE (the same check for the device-bound setters is in test_gpu_lrc_ranks.py).
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from parmgmc_amd.capi import lib
from test_lrc import ball_matrix, observation_matrix

ARG_OUTOFRANGE = 63


def _split_in_colour_order(A, colors):
    """(M, N, perm): A = M - N with M = D + L of A permuted so that the colours come one after the other (rows of one
    colour in ascending order) -- the matrix one forward multicolour sweep with omega = 1 inverts"""
    perm = np.argsort(colors, kind="stable")
    Ap = A.dense()[np.ix_(perm, perm)]
    M = np.tril(Ap)
    return M, M - Ap, perm


@pytest.mark.parametrize("grid,kind", [((7, 6, 3), "balls"), ((6, 6, 2), "wide")])
def test_oracle_lrc_sweep_is_one_sor_step_on_the_explicit_sum_at_k64(grid, kind):
    """Sherman-Morrison-Woodbury: the forward sweep on A followed by y -= Bb (B^T y), Bb = M^-1 B (S^-1 + B^T M^-1 B)^-1,
    equals a Gauss-Seidel step on M + B S B^T.  k = 64 > n / 4: B has more columns than a quarter of the rows, one of
    them zero (an empty ball)"""
    k = 64
    A = O.shifted_laplace(*grid, 2.0)
    n = A.n
    col = O.coloring_redblack(*grid)
    if kind == "balls":
        rng = np.random.default_rng(7)
        centres = [tuple(rng.uniform(0, 1, 3)) for _ in range(k)]
        radii = list(rng.uniform(0.3, 0.45, k))
        radii[17] = 0.0  # an empty ball: a zero column of B
        B = ball_matrix(grid, centres, radii)
        assert not B[:, 17].any() and np.count_nonzero(np.abs(B).sum(0)) == k - 1
    else:
        B = observation_matrix(n, k, 3)
    S = np.linspace(5.0, 90.0, k)
    rng = np.random.default_rng(11)
    b, y = rng.standard_normal(n), rng.standard_normal(n)
    Bb_f = O.lrc_build_correction(A, col, B, S, 1.0, O.SOR_FORWARD)
    Bb_b = O.lrc_build_correction(A, col, B, S, 1.0, O.SOR_BACKWARD)
    got = O.lrc_mcsor_apply(A, col, B, Bb_f, Bb_b, b, y, 1.0, O.SOR_FORWARD)

    M, N, p = _split_in_colour_order(A, col)
    Bp = B[p]
    want = np.empty(n)
    want[p] = np.linalg.solve(M + Bp @ np.diag(S) @ Bp.T, b[p] + N @ y[p])
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-12
    # the plain sweep is the same step without the update, and the update is not lost in the tolerance
    plain = np.empty(n)
    plain[p] = np.linalg.solve(M, b[p] + N @ y[p])
    assert np.allclose(O.mcsor_apply(A, col, b, y, 1.0, O.SOR_FORWARD), plain, rtol=1e-12, atol=1e-13)
    assert np.abs(plain - want).max() / np.abs(want).max() > 1e-6
    # ... nor is the last column's
    S2 = S.copy()
    S2[63] *= 1.5
    other = np.empty(n)
    other[p] = np.linalg.solve(M + Bp @ np.diag(S2) @ Bp.T, b[p] + N @ y[p])
    assert np.abs(other - want).max() / np.abs(want).max() > 1e-8


def _lap1d(n):
    rows, cols, vals = [], [], []
    for i in range(n):
        for j, v in ((i - 1, -1.0), (i, 2.5), (i + 1, -1.0)):
            if 0 <= j < n:
                rows.append(i), cols.append(j), vals.append(v)
    rp = np.zeros(n + 1, np.int32)
    np.add.at(rp, np.array(rows) + 1, 1)
    return np.cumsum(rp).astype(np.int32), np.array(cols, np.int32), np.array(vals)


@pytest.mark.parametrize("k", [-1, 65])
def test_rank_out_of_range_is_rejected_before_any_device_work(k):
    n = 8
    rp, ci, v = _lap1d(n)
    B, S = np.ones((n, 70), order="F"), np.ones(70)  # large enough for any rank a check might let through
    out = C.c_void_p()
    # the exact coarse sampler of A + B S B^T (32- and 64-bit index entry points)
    assert lib.pmg_chol_create_csr_lowrank(n, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, k, B.ctypes.data, S.ctypes.data, C.byref(out)) == ARG_OUTOFRANGE
    assert not out.value
    rp64, ci64 = rp.astype(np.int64), ci.astype(np.int64)
    assert lib.pmg_chol_create_csr_idx(n, rp64.ctypes.data, ci64.ctypes.data, v.ctypes.data, 64, k, B.ctypes.data, S.ctypes.data, C.byref(out)) == ARG_OUTOFRANGE
    assert not out.value
    # PCWOODBURY
    assert lib.pmg_woodbury_create(n, k, B.ctypes.data, n, S.ctypes.data, None, C.byref(out)) == ARG_OUTOFRANGE
    assert not out.value
    # MatCreateLRC
    m = C.c_void_p()
    assert lib.pmg_mat_create_csr(n, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, C.byref(m)) == 0
    assert lib.pmg_mat_create_lrc(m, k, B.ctypes.data, S.ctypes.data, C.byref(out)) == ARG_OUTOFRANGE
    assert not out.value
    assert lib.pmg_mat_destroy(C.byref(m)) == 0
    # MGMC on a caller-supplied hierarchy and on a DMDA grid (both host-only until set-up)
    h = C.c_void_p()
    rpc, cic, vc = _lap1d(n // 2)
    prp, pci, pv = np.arange(n + 1, dtype=np.int32), (np.arange(n) // 2).astype(np.int32), np.ones(n)
    assert lib.pmg_mgmc_create_hierarchy(2, C.byref(h)) == 0
    assert lib.pmg_mgmc_set_level_operator(h, 0, n // 2, rpc.ctypes.data, cic.ctypes.data, vc.ctypes.data) == 0
    assert lib.pmg_mgmc_set_level_operator(h, 1, n, rp.ctypes.data, ci.ctypes.data, v.ctypes.data) == 0
    assert lib.pmg_mgmc_set_level_interpolation(h, 1, n, n // 2, prp.ctypes.data, pci.ctypes.data, pv.ctypes.data) == 0
    assert lib.pmg_mgmc_set_lowrank(h, k, B.ctypes.data, S.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_mgmc_destroy(C.byref(h)) == 0
    assert lib.pmg_mgmc_create_dmda(9, 9, 1, 1.0, 2, C.byref(h)) == 0
    Bg = np.ones((81, 70), order="F")
    assert lib.pmg_mgmc_set_lowrank(h, k, Bg.ctypes.data, S.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_mgmc_destroy(C.byref(h)) == 0


def test_rank_range_ends_are_accepted_where_no_device_is_needed():
    """k = 1 and k = 64 pass the same checks (the MGMC setter only stores the factors until set-up)"""
    h = C.c_void_p()
    assert lib.pmg_mgmc_create_dmda(9, 9, 1, 1.0, 2, C.byref(h)) == 0
    B, S = np.ones((81, 64), order="F"), np.ones(64)
    for k in (1, 64, 0):
        assert lib.pmg_mgmc_set_lowrank(h, k, B.ctypes.data, S.ctypes.data) == 0
    assert lib.pmg_mgmc_destroy(C.byref(h)) == 0
    m, out = C.c_void_p(), C.c_void_p()
    rp, ci, v = _lap1d(8)
    assert lib.pmg_mat_create_csr(8, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, C.byref(m)) == 0
    assert lib.pmg_mat_create_lrc(m, 64, B.ctypes.data, S.ctypes.data, C.byref(out)) == 0
    assert lib.pmg_mat_destroy(C.byref(out)) == 0
    assert lib.pmg_mat_destroy(C.byref(m)) == 0
