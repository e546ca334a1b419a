"""CPU checks of the references in chol_edge_refs.py (used by test_gpu_chol_edges.py) and the size limit of the dense
coarse sampler, which is refused before anything touches a device."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from chol_edge_refs import (
    LD_FULL_MAX,
    dense_spd,
    eig_range,
    factor_bound,
    factor_error,
    fwd_bound,
    lapack_info,
    mp_sample,
    noise_bound,
    noise_error,
    rel_inf,
    solve_ref,
    with_failing_minor,
)

MINOR_ORDERS = [1, 2, 31, 32, 33, 64, 65, 97, 129]


def test_mpmath_sample_and_refined_solve_agree():
    A = dense_spd(33, 1e6, 3)
    lo, hi = eig_range(A)
    b = np.random.default_rng(4).standard_normal(33)
    x = solve_ref(A, b)
    assert rel_inf(x, mp_sample(A, b, None)) <= 4 * 2.0**-53 * 33  # refined: close to u, not kappa u
    xi = O.noise_rows(33, 7, 2)
    y = mp_sample(A, b, xi)
    e = rel_inf(O.chol_sample(O.potrf_lower(A), b, xi), y)
    assert e <= fwd_bound(33, hi / lo)
    # negative control: the next counter's noise is another sample
    assert rel_inf(O.chol_sample(O.potrf_lower(A), b, O.noise_rows(33, 7, 3)), y) > fwd_bound(33, hi / lo)


@pytest.mark.parametrize("n", [65, LD_FULL_MAX + 30])
def test_factor_error_of_lapack_meets_the_bound(n, monkeypatch):
    A = dense_spd(n, 1e6, n)
    L = np.linalg.cholesky(A)
    e = factor_error(A, L)
    assert 0 < e <= factor_bound(A)
    if n <= LD_FULL_MAX:  # the probe estimate is within a small factor of the exact norm
        import chol_edge_refs as R

        monkeypatch.setattr(R, "LD_FULL_MAX", 0)
        assert 0.3 < R.factor_error(A, L) / e < 3
    # negative control: one entry of the far-off-diagonal tile 1e-8 off
    blk = np.abs(L[n - (n % 32 or 32) :, :32])
    i, j = np.unravel_index(np.argmax(blk), blk.shape)
    Lb = L.copy()
    Lb[n - (n % 32 or 32) + i, j] *= 1 + 1e-8
    assert factor_error(A, Lb) > factor_bound(A)


def test_noise_invariant_of_the_oracle_sample():
    A = dense_spd(97, 1e6, 5)
    lo, hi = eig_range(A)
    L = O.potrf_lower(A)
    b = np.sqrt(lo) * np.random.default_rng(6).standard_normal(97)
    xi = O.noise_rows(97, 1, 0)
    z = O.chol_sample(L, b, xi) - O.chol_sample(L, b, np.zeros(97))
    assert noise_error(L, z, xi) <= noise_bound(97, hi / lo)
    assert noise_error(L, z, O.noise_rows(97, 1, 1)) > noise_bound(97, hi / lo)


def test_failing_minor_construction_matches_lapack():
    """(a NaN pivot is not pinned to dpotrf here: reference LAPACK's dpotrf2 reports it, OpenBLAS's own dpotrf, which scipy
    may use, tests only ajj <= 0 and returns 0)"""
    A = dense_spd(129, 1e3, 8)
    assert lapack_info(A) == 0
    for m in MINOR_ORDERS:
        assert lapack_info(with_failing_minor(A, m)) == m
    for r in (0, 32, 128):  # an empty row of the lower triangle: pivot 0 at order r + 1
        Bz = A.copy()
        Bz[r, :] = 0.0
        assert lapack_info(Bz) == r + 1


def test_dense_sampler_size_limit_refused_before_device_work():
    """pmg_chol_create_csr_lowrank refuses npad^2 * 32 bytes >= 96e9 (PETSC_ERR_SUP, 56) before it allocates: on a machine
    without a GPU any device call would fail with another code.  n = 54753 is the smallest refused size (npad = 54784;
    npad = 54752 is accepted)."""
    from parmgmc_amd.capi import lib

    assert 54752**2 * 32 < 96e9 <= 54784**2 * 32
    n = 54753
    rp, ci, v = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n)
    h = C.c_void_p()
    assert lib.pmg_chol_create_csr(n, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, C.byref(h)) == 56
    assert b"dense coarse sampler limited" in lib.pmg_last_error_string() and not h.value
    assert lib.pmg_chol_create_csr_lowrank(n, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 0, None, None, C.byref(h)) == 56
    assert not h.value
