"""The chain-covariance group (pmg_chaincov_*) is declared, bound and exported, and rejects bad calls before any device work.
CPU only: every call here returns before the device is touched."""
import ctypes as C

import numpy as np

from parmgmc_amd import capi
from parmgmc_amd.capi import lib

ARG_NULL, ARG_OUTOFRANGE, ARG_SIZ, SUP = 85, 63, 60, 56
NEW = ["pmg_chaincov_create_chol", "pmg_chaincov_create_dense", "pmg_chaincov_destroy", "pmg_chaincov_set_stream", "pmg_chaincov_update", "pmg_chaincov_callback",
       "pmg_chaincov_reset", "pmg_chaincov_get_count", "pmg_chaincov_get_errors", "pmg_chaincov_get_reference", "pmg_chaincov_covariance"]


def test_new_symbols_are_exported_and_declared():
    declared = capi.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi._sig, name
    import parmgmc_amd

    assert hasattr(parmgmc_amd, "ChainCov")
    for m in ("from_chol", "from_csr", "from_dense", "update", "errors", "reference", "covariance", "reset", "count"):
        assert hasattr(parmgmc_amd.ChainCov, m), m


def _handle(n=10, nchains=4, max_steps=3):
    h = C.c_void_p()
    S = np.eye(n)
    assert lib.pmg_chaincov_create_dense(n, S.ctypes.data, nchains, max_steps, C.byref(h)) == 0  # allocates nothing on the device
    return h


def test_create_argument_checks():
    h = C.c_void_p()
    S = np.eye(10)
    assert lib.pmg_chaincov_create_dense(10, S.ctypes.data, 4, 5, None) == ARG_NULL
    assert lib.pmg_chaincov_create_dense(10, None, 4, 5, C.byref(h)) == ARG_NULL
    assert lib.pmg_chaincov_create_dense(0, S.ctypes.data, 4, 5, C.byref(h)) == ARG_OUTOFRANGE
    assert lib.pmg_chaincov_create_dense(-3, S.ctypes.data, 4, 5, C.byref(h)) == ARG_OUTOFRANGE
    # above the host function's limit: its code and its message; the matrix (far too small here) is never read
    assert lib.pmg_chaincov_create_dense(4097, S.ctypes.data, 4, 5, C.byref(h)) == SUP
    assert b"dense covariance diagnostics are meant for small problems (n = 4097)" in lib.pmg_last_error_string()
    assert lib.pmg_chaincov_create_dense(10, S.ctypes.data, 1, 5, C.byref(h)) == ARG_OUTOFRANGE  # as pmg_estimate_covariance_errors
    assert lib.pmg_chaincov_create_dense(10, S.ctypes.data, 0, 5, C.byref(h)) == ARG_OUTOFRANGE
    assert lib.pmg_chaincov_create_dense(10, S.ctypes.data, 4, 0, C.byref(h)) == ARG_OUTOFRANGE
    assert not h.value
    # the Cholesky constructor: NULLs are refused before the handle is looked at
    assert lib.pmg_chaincov_create_chol(None, 4, 5, C.byref(h)) == ARG_NULL
    assert lib.pmg_chaincov_create_chol(C.c_void_p(0x2000), 4, 5, None) == ARG_NULL
    assert not h.value
    for nchains in (2, 1000):
        assert lib.pmg_chaincov_create_dense(10, S.ctypes.data, nchains, 1, C.byref(h)) == 0 and h.value
        assert lib.pmg_chaincov_destroy(C.byref(h)) == 0 and not h.value
    assert lib.pmg_chaincov_destroy(C.byref(h)) == 0  # destroying NULL is a no-op
    assert lib.pmg_chaincov_destroy(None) == 0


def test_host_function_agrees_on_the_limits():
    """the codes above are pmg_estimate_covariance_errors' own"""
    rp, ci, v = np.arange(3, dtype=np.int32), np.arange(2, dtype=np.int32), np.ones(2)
    S, e = np.zeros(4), np.zeros(1)
    assert lib.pmg_estimate_covariance_errors(2, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 1, 1, S.ctypes.data, e.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_estimate_covariance_errors(4097, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 2, 1, S.ctypes.data, e.ctypes.data) == SUP


def test_argument_checks_before_the_device():
    h = _handle()
    Y = C.c_void_p(0x2000)  # never dereferenced: every call below fails its checks first
    out = np.zeros(128)
    st = C.c_int32(-1)
    assert lib.pmg_chaincov_update(None, Y, None) == ARG_NULL
    assert lib.pmg_chaincov_update(h, None, None) == ARG_NULL
    assert lib.pmg_chaincov_callback(0, Y, 10, 4, None) == ARG_NULL
    assert lib.pmg_chaincov_callback(0, Y, 11, 4, h) == ARG_SIZ
    assert lib.pmg_chaincov_callback(0, Y, 10, 3, h) == ARG_SIZ
    assert lib.pmg_chaincov_callback(0, None, 10, 4, h) == ARG_NULL
    assert lib.pmg_chaincov_covariance(None, Y, Y, None) == ARG_NULL
    assert lib.pmg_chaincov_covariance(h, None, Y, None) == ARG_NULL
    assert lib.pmg_chaincov_covariance(h, Y, None, None) == ARG_NULL
    assert lib.pmg_chaincov_set_stream(None, None) == ARG_NULL
    assert lib.pmg_chaincov_set_stream(h, None) == 0
    assert lib.pmg_chaincov_get_count(None, C.byref(st)) == ARG_NULL
    assert lib.pmg_chaincov_get_count(h, None) == ARG_NULL
    assert lib.pmg_chaincov_get_count(h, C.byref(st)) == 0 and st.value == 0
    assert lib.pmg_chaincov_reset(None) == ARG_NULL
    assert lib.pmg_chaincov_reset(h) == 0
    # the recorded window is empty
    assert lib.pmg_chaincov_get_errors(None, 0, 0, out.ctypes.data) == ARG_NULL
    assert lib.pmg_chaincov_get_errors(h, 0, 1, out.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_chaincov_get_errors(h, -1, 0, out.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_chaincov_get_errors(h, 0, -1, out.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_chaincov_get_errors(h, 1, 0, out.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_chaincov_get_errors(h, 0, 0, out.ctypes.data) == 0  # the empty window
    assert lib.pmg_chaincov_get_reference(None, out.ctypes.data) == ARG_NULL
    assert lib.pmg_chaincov_get_reference(h, None) == ARG_NULL
    assert lib.pmg_chaincov_destroy(C.byref(h)) == 0


def test_reference_of_a_dense_handle_before_any_update():
    """create_dense copies the matrix; it is readable without a device until the first update uploads it"""
    rng = np.random.default_rng(0)
    M = rng.standard_normal((7, 7))
    S = M @ M.T
    h = C.c_void_p()
    assert lib.pmg_chaincov_create_dense(7, S.ctypes.data, 3, 2, C.byref(h)) == 0
    keep = S.copy()
    S[:] = 0.0  # the handle holds its own copy
    out = np.empty((7, 7))
    assert lib.pmg_chaincov_get_reference(h, out.ctypes.data) == 0
    assert np.array_equal(out, keep)
    assert lib.pmg_chaincov_destroy(C.byref(h)) == 0


def test_wrapper_refuses_cov_with_callback_and_other_sizes():
    import pytest

    from parmgmc_amd import ChainCov
    from parmgmc_amd.capi import PMGError

    cc = ChainCov.from_dense(np.eye(5), nchains=3, max_steps=2)
    assert (cc.n, cc.nchains, cc.count()) == (5, 3, 0)
    assert cc.errors().shape == (0,)
    with pytest.raises(AssertionError):
        cc._as_callback(5, 4)
    with pytest.raises(PMGError):
        ChainCov.from_dense(np.eye(5), nchains=1)
    cc.destroy()
