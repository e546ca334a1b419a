"""The device IACT entry points (pmg_iact_chains, pmg_chainstats_iact) are declared, bound and exported, and reject bad calls
with the reference's code and message before any device work.  CPU only: every call here returns before the device is touched."""
import ctypes as C

import numpy as np

from parmgmc_amd import capi
from parmgmc_amd.capi import lib

ARG_NULL, ARG_OUTOFRANGE = 85, 63
NEW = ["pmg_iact_chains", "pmg_chainstats_iact"]
X = C.c_void_p(0x2000)  # never dereferenced: every call below fails its checks first
ACF = C.c_void_p(0x4000)


def test_new_symbols_are_exported_and_declared():
    declared = capi.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi._sig, name
    import parmgmc_amd

    assert hasattr(parmgmc_amd, "iact_chains") and hasattr(parmgmc_amd.ChainStats, "iact_device")
    assert 64 <= parmgmc_amd.IACT_LAG_BLOCK <= 512
    text = capi.header_path().read_text()
    assert f"#define PMG_IACT_LAG_BLOCK {parmgmc_amd.IACT_LAG_BLOCK}\n" in text


def _out(S=4):
    return np.full(S, -7.0), np.full(S, -7, np.int32), np.full(S, -7, np.int32)


def _untouched(tau, win, val):
    return (tau == -7.0).all() and (win == -7).all() and (val == -7).all()


def test_iact_chains_argument_checks():
    tau, win, val = _out()
    t, w, v = tau.ctypes.data, win.ctypes.data, val.ctypes.data
    assert lib.pmg_iact_chains(100, 4, None, 4, 0, t, w, v, 0, None, None) == ARG_NULL
    assert lib.pmg_iact_chains(100, 4, X, 4, 0, None, w, v, 0, None, None) == ARG_NULL
    for n in (1, 0, -3):
        assert lib.pmg_iact_chains(n, 4, X, 4, 0, t, w, v, 0, None, None) == ARG_OUTOFRANGE
        assert b"Too few data points" in lib.pmg_last_error_string()  # src/iact.c:79
    assert lib.pmg_iact_chains(1 << 31, 1, X, 1, 0, t, w, v, 0, None, None) == ARG_OUTOFRANGE  # the window is a 32-bit lag
    for S in (0, -1):
        assert lib.pmg_iact_chains(100, S, X, 4, 0, t, w, v, 0, None, None) == ARG_OUTOFRANGE
        assert b"nseries" in lib.pmg_last_error_string()
    assert lib.pmg_iact_chains(1 << 30, 1 << 20, X, 1 << 20, 0, t, w, v, 0, None, None) == ARG_OUTOFRANGE  # the scratch
    assert lib.pmg_iact_chains(100, 4, X, 3, 0, t, w, v, 0, None, None) == ARG_OUTOFRANGE
    assert b"leading dimension" in lib.pmg_last_error_string()
    assert lib.pmg_iact_chains(100, 4, X, 4, -1, t, w, v, 0, None, None) == ARG_OUTOFRANGE
    assert b"max_lag" in lib.pmg_last_error_string()
    for nacf in (-1, 101):
        assert lib.pmg_iact_chains(100, 4, X, 4, 0, t, w, v, nacf, ACF, None) == ARG_OUTOFRANGE
        assert b"nacf" in lib.pmg_last_error_string()
    assert _untouched(tau, win, val)


def _handle(n=10, nchains=4, nqoi=2, max_steps=30):
    h = C.c_void_p()
    assert lib.pmg_chainstats_create(n, nchains, nqoi, max_steps, C.byref(h)) == 0  # allocates nothing on the device
    return h


def test_chainstats_iact_argument_checks():
    tau, win, val = _out()
    t, w, v = tau.ctypes.data, win.ctypes.data, val.ctypes.data
    h = _handle()
    assert lib.pmg_chainstats_iact(None, 0, 0, 2, 0, t, w, v, 0, None, None) == ARG_NULL
    assert lib.pmg_chainstats_iact(h, 0, 0, 2, 0, None, w, v, 0, None, None) == ARG_NULL
    for q in (-1, 2):
        assert lib.pmg_chainstats_iact(h, q, 0, 0, 0, t, w, v, 0, None, None) == ARG_OUTOFRANGE
        assert b"QOI" in lib.pmg_last_error_string()
    # nothing has been recorded: every window but the empty one lies outside, and the empty one has too few points
    for first, count in ((0, 2), (0, 30), (1, 0), (-1, 2), (0, -1)):
        assert lib.pmg_chainstats_iact(h, 0, first, count, 0, t, w, v, 0, None, None) == ARG_OUTOFRANGE
        assert b"recorded" in lib.pmg_last_error_string()
    assert lib.pmg_chainstats_iact(h, 0, 0, 0, 0, t, w, v, 0, None, None) == ARG_OUTOFRANGE
    assert b"Too few data points" in lib.pmg_last_error_string()
    assert lib.pmg_chainstats_iact(h, 1, 0, 0, -1, t, w, v, 5, ACF, None) == ARG_OUTOFRANGE  # the count comes first
    assert b"Too few data points" in lib.pmg_last_error_string()
    assert lib.pmg_chainstats_destroy(C.byref(h)) == 0
    h = _handle(nqoi=0)  # a handle without QOI has no trace
    assert lib.pmg_chainstats_iact(h, 0, 0, 0, 0, t, w, v, 0, None, None) == ARG_OUTOFRANGE
    assert b"QOI" in lib.pmg_last_error_string()
    assert lib.pmg_chainstats_destroy(C.byref(h)) == 0
    assert _untouched(tau, win, val)
