"""The matrix-free Rao-Blackwellised statistics handle on a DMDA grid (pmg_rbstats_create_dmda) without a device: the symbol is
declared, exported and bound; every argument check returns its status in the documented order; the conditional precisions are
the diagonal of oracle.shifted_laplace bit for bit (and, with a low-rank term, those of the CSR handle on that matrix); the byte
model is the documented formula; and the host code runs clean under AddressSanitizer and UndefinedBehaviorSanitizer in a
stand-alone program (tests/sanitize/rbstats_dmda_host.c, nothing preloaded).
CPU only: every call here returns before the device is touched."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle as O

ROOT = Path(__file__).resolve().parent.parent
ARG_NULL, ARG_OUTOFRANGE, ARG_WRONGSTATE, ARG_SIZ, ARG_WRONG = 85, 63, 73, 60, 62
GRIDS = [(2, 2, 1), (5, 4, 3), (9, 9, 1), (17, 17, 17)]
KAPPA = 0.1  # 0.1 * 0.1 is not a float64: the product is rounded, and so is every sum on top of it


def _lib():
    from parmgmc_amd.capi import lib

    return lib


def _create(nx, ny, nz, kappa=KAPPA, nchains=1):
    h = C.c_void_p()
    st = _lib().pmg_rbstats_create_dmda(nx, ny, nz, kappa, nchains, C.byref(h))
    return st, h


def _csr_handle(A, nchains=1):
    h = C.c_void_p()
    assert _lib().pmg_rbstats_create_csr(A.n, A.rowptr.ctypes.data, A.colidx.ctypes.data, A.vals.ctypes.data, nchains, C.byref(h)) == 0
    return h


def _q(h, n):
    q = np.full(n + 1, -7.0)  # one sentinel behind the n entries
    assert _lib().pmg_rbstats_get_cond_precision(h, q.ctypes.data) == 0
    assert q[n] == -7.0
    return q[:n]


def _diagonal(A):
    return np.array([A.vals[j] for i in range(A.n) for j in range(A.rowptr[i], A.rowptr[i + 1]) if A.colidx[j] == i])


def test_symbol_is_declared_exported_and_bound():
    from parmgmc_amd import RBStats, capi

    assert "pmg_rbstats_create_dmda" in capi.declared_symbols()
    assert hasattr(capi.lib, "pmg_rbstats_create_dmda")
    assert "pmg_rbstats_create_dmda" in capi._sig
    assert callable(RBStats.dmda)


def test_create_checks_in_order():
    lib = _lib()
    assert lib.pmg_rbstats_create_dmda(0, 4, 3, KAPPA, 0, None) == ARG_NULL  # the out-pointer before everything else
    h = C.c_void_p(0x10)
    assert lib.pmg_rbstats_create_dmda(1, 4, 3, KAPPA, 1, C.byref(h)) == ARG_OUTOFRANGE and not h.value  # nx < 2; *rb is cleared
    for grid in [(1, 1, 1), (-3, 4, 4), (5, 0, 3), (5, 4, 0), (5, -1, 3), (5, 4, -1)]:
        st, h = _create(*grid, nchains=0)  # the grid before the chains
        assert st == ARG_OUTOFRANGE and not h.value and b"grid" in lib.pmg_last_error_string(), grid
    # products that do not fit 32 bits: 2^31, 2^32 (0 when it wraps), 2^33 with an x-y plane that fits, and the largest sizes
    for grid in [(2048, 2048, 512), (65536, 65536, 1), (65536, 2, 65536), (2, 2, 2**30), (2**31 - 1, 2**31 - 1, 2**31 - 1)]:
        st, h = _create(*grid, nchains=0)  # the size before the chains
        assert st == ARG_OUTOFRANGE and not h.value and b"points" in lib.pmg_last_error_string(), grid
    for nchains in (0, -1, -(2**31)):
        st, h = _create(5, 4, 3, nchains=nchains)
        assert st == ARG_OUTOFRANGE and not h.value and b"nchains" in lib.pmg_last_error_string()
    for kappa in (np.nan, np.inf, 1e200):
        st, h = _create(5, 4, 3, kappa=kappa)
        assert st == ARG_WRONG and not h.value and b"positive and finite" in lib.pmg_last_error_string()
    assert lib.pmg_rbstats_destroy(C.byref(h)) == 0  # destroying what a failed creation left is a no-op
    for nchains in (1, 64, 1000):
        st, h = _create(5, 4, 3, nchains=nchains)
        assert st == 0 and h.value
        assert lib.pmg_rbstats_destroy(C.byref(h)) == 0 and not h.value
    st, h = _create(2, 1, 1, kappa=0.0)  # kappa = 0 is a valid operator here: every point has a neighbour
    assert st == 0 and np.array_equal(_q(h, 2), [1.0, 1.0])
    assert lib.pmg_rbstats_destroy(C.byref(h)) == 0


def test_checks_of_the_shared_entry_points_before_the_device():
    lib = _lib()
    st, h = _create(5, 4, 3, nchains=4)
    assert st == 0
    n = 60
    Y, M = C.c_void_p(0x2000), C.c_void_p(0x4000)  # never dereferenced
    B, S = np.asfortranarray(np.ones((n, 2))), np.ones(2)
    q0 = _q(h, n).copy()
    assert lib.pmg_rbstats_set_lowrank(h, -1, B.ctypes.data, S.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_rbstats_set_lowrank(h, 65, B.ctypes.data, S.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_rbstats_set_lowrank(h, 2, None, S.ctypes.data) == ARG_NULL
    assert lib.pmg_rbstats_set_lowrank(h, 2, B.ctypes.data, None) == ARG_NULL
    assert lib.pmg_rbstats_set_lowrank(h, 2, B.ctypes.data, (-5.0 * S).ctypes.data) == ARG_WRONG  # q < 0
    Binf = B.copy(order="F")
    Binf[7, 1] = 1e200  # B * B overflows: q = inf
    assert lib.pmg_rbstats_set_lowrank(h, 2, Binf.ctypes.data, S.ctypes.data) == ARG_WRONG
    Bnan = B.copy(order="F")
    Bnan[n - 1, 0] = np.nan
    assert lib.pmg_rbstats_set_lowrank(h, 2, Bnan.ctypes.data, S.ctypes.data) == ARG_WRONG
    assert np.array_equal(_q(h, n), q0)  # the rejected terms changed nothing
    assert lib.pmg_rbstats_set_lowrank(h, 2, B.ctypes.data, S.ctypes.data) == 0  # host copies only
    assert np.array_equal(_q(h, n), q0 + 1.0 + 1.0)
    assert lib.pmg_rbstats_set_lowrank(h, 0, None, None) == 0
    assert np.array_equal(_q(h, n), q0)
    assert lib.pmg_rbstats_update(h, None, None) == ARG_NULL
    assert lib.pmg_rbstats_cond_mean(h, Y, None, None) == ARG_NULL
    assert lib.pmg_rbstats_cond_mean(h, Y, Y, None) == ARG_WRONG
    assert lib.pmg_rbstats_callback(0, Y, n - 20, 4, h) == ARG_SIZ  # the rows of a z-slab: fewer than the handle has
    assert lib.pmg_rbstats_callback(0, Y, n, 3, h) == ARG_SIZ
    assert lib.pmg_rbstats_sample_callback(0, Y, n, h) == ARG_SIZ  # a handle of 4 chains on a single-chain sampler
    assert lib.pmg_rbstats_get_fields(h, Y, M, None) == ARG_WRONGSTATE
    st_, sm = C.c_int32(-1), C.c_int64(-1)
    assert lib.pmg_rbstats_reset(h) == 0
    assert lib.pmg_rbstats_get_count(h, C.byref(st_), C.byref(sm)) == 0 and (st_.value, sm.value) == (0, 0)
    assert lib.pmg_rbstats_destroy(C.byref(h)) == 0


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_cond_precision_is_the_assembled_diagonal_bit_for_bit(grid):
    lib = _lib()
    assert KAPPA * KAPPA != 0.01  # the product rounds
    A = O.shifted_laplace(*grid, KAPPA)
    n = A.n
    st, h = _create(*grid)
    assert st == 0
    want = _diagonal(A)
    assert len(want) == n and np.array_equal(_q(h, n), want)
    # with a B of rank 3: the q of the CSR handle on the assembled operator
    rng = np.random.default_rng(n)
    B, S = np.asfortranarray(rng.uniform(-1.0, 1.0, (n, 3)) / np.sqrt(n)), rng.uniform(0.5, 20.0, 3)
    B[n // 2] = 0.0
    hc = _csr_handle(A)
    for hh in (h, hc):
        assert lib.pmg_rbstats_set_lowrank(hh, 3, B.ctypes.data, S.ctypes.data) == 0
    q, qc = _q(h, n), _q(hc, n)
    assert np.array_equal(q, qc) and (q >= want).all() and (q > want).any() and q[n // 2] == want[n // 2]
    hand = want.copy()
    for k in range(3):
        hand = hand + S[k] * (B[:, k] * B[:, k])
    assert np.array_equal(q, hand)
    assert lib.pmg_rbstats_set_lowrank(h, 0, None, None) == 0
    assert np.array_equal(_q(h, n), want)
    assert lib.pmg_rbstats_destroy(C.byref(h)) == 0 and lib.pmg_rbstats_destroy(C.byref(hc)) == 0


@pytest.mark.parametrize("nchains", [1, 3, 65])
@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("k", [0, 3])
def test_byte_model(k, with_b, nchains):
    """8 n C (Y once) + 32 n (mean and M2, read and written) + 8 n with a right-hand side + 8 n (q) + 8 n k (B) + 8 n C (Y once
    more, for B^T Y) with a low-rank term; no term for a matrix, which the CSR handle on the same operator has"""
    lib = _lib()
    nx, ny, nz = 5, 4, 3
    n = nx * ny * nz
    st, h = _create(nx, ny, nz, nchains=nchains)
    assert st == 0
    if k:
        B, S = np.asfortranarray(np.full((n, k), 0.25)), np.ones(k)
        assert lib.pmg_rbstats_set_lowrank(h, k, B.ctypes.data, S.ctypes.data) == 0
    assert lib.pmg_rbstats_set_rhs(h, C.c_void_p(0x2000) if with_b else None) == 0  # borrowed, not read
    by = C.c_double(-1.0)
    assert lib.pmg_rbstats_get_algorithmic_bytes(h, C.byref(by)) == 0
    want = 8 * n * nchains + 32 * n + (8 * n if with_b else 0) + ((8 * n + 8 * n * k + 8 * n * nchains) if k else 0)
    assert by.value == want
    A = O.shifted_laplace(nx, ny, nz, KAPPA)
    hc = _csr_handle(A, nchains)
    assert lib.pmg_rbstats_get_algorithmic_bytes(hc, C.byref(by)) == 0
    assert by.value == 12 * len(A.vals) + 8 * n * nchains + 48 * n  # unchanged
    assert lib.pmg_rbstats_destroy(C.byref(h)) == 0 and lib.pmg_rbstats_destroy(C.byref(hc)) == 0


def test_byte_model_at_the_size_the_issue_quotes():
    """257^3, one chain, b set: 48 B per unknown, 0.81 GB, against 2.37 GB of the CSR handle's model (118 M stored entries)"""
    lib = _lib()
    n = 257**3
    st, h = _create(257, 257, 257)
    assert st == 0
    assert lib.pmg_rbstats_set_rhs(h, C.c_void_p(0x2000)) == 0
    by = C.c_double()
    assert lib.pmg_rbstats_get_algorithmic_bytes(h, C.byref(by)) == 0 and by.value == 48.0 * n
    nnz = n + 2 * 3 * 256 * 257 * 257
    assert round((12.0 * nnz + 8.0 * n + 48.0 * n) / by.value, 1) == 2.9
    assert lib.pmg_rbstats_destroy(C.byref(h)) == 0


def test_python_mirror_without_a_device():
    from parmgmc_amd import RBStats

    rb = RBStats.dmda(5, 4, 3, KAPPA, nchains=2)
    assert (rb.n, rb.nchains, rb.k) == (60, 2, 0) and rb.count() == (0, 0)
    assert np.array_equal(rb.cond_precision(), _diagonal(O.shifted_laplace(5, 4, 3, KAPPA)))
    rb.set_lowrank(np.full((60, 2), 0.5), np.array([1.0, 2.0]))
    assert rb.k == 2 and rb.algorithmic_bytes() == 8 * 60 * 2 + 32 * 60 + 8 * 60 + 8 * 60 * 2 + 8 * 60 * 2
    rb.destroy()


def test_host_part_under_sanitizers(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    exe = tmp_path / "rbstats_dmda_host"
    csrc = ROOT / "parmgmc_amd" / "csrc"
    srcs = [ROOT / "tests" / "sanitize" / "rbstats_dmda_host.c", csrc / "pmg_rbstats.c", csrc / "pmg_chains_common.c"]
    cmd = [gcc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", *map(str, srcs), "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}, timeout=120)
    assert run.returncode == 0 and run.stdout.endswith("rbstats_dmda_host ok\n"), (run.stdout[-2000:], run.stderr[-4000:])
