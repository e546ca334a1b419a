"""Posterior sampling on many chains: the per-chain right-hand-side entry points (pmg_mcsor_sample_chains_rhs,
pmg_mgmc_sample_chains_rhs) and the Woodbury chain calls (pmg_woodbury_noisy_rhs_chains, pmg_woodbury_correct_chains) are
exported, declared, and reject bad calls before any device work; so do pmg_woodbury_create's argument checks and the null
handles of every other pmg_woodbury_* call.  CPU only: every call here returns before the device is touched.  (The state
checks of a Woodbury handle need one, which lives on the device: tests/test_gpu_woodbury_term.py.)"""
import ctypes as C

import numpy as np

from parmgmc_amd import capi
from parmgmc_amd.capi import lib

ARG_NULL, ARG_OUTOFRANGE, ARG_WRONGSTATE = 85, 63, 73
NEW = ["pmg_mcsor_sample_chains_rhs", "pmg_mgmc_sample_chains_rhs", "pmg_woodbury_noisy_rhs_chains", "pmg_woodbury_correct_chains"]


def _lap1d(n):
    """CSR of the shifted 1-D Laplacian tridiag(-1, 2.5, -1)"""
    rows, cols, vals = [], [], []
    for i in range(n):
        for j, v in ((i - 1, -1.0), (i, 2.5), (i + 1, -1.0)):
            if 0 <= j < n:
                rows.append(i), cols.append(j), vals.append(v)
    rp = np.zeros(n + 1, np.int32)
    np.add.at(rp, np.array(rows) + 1, 1)
    return np.cumsum(rp).astype(np.int32), np.array(cols, np.int32), np.array(vals)


def test_new_symbols_are_exported_and_declared():
    declared = capi.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi._sig, name


def test_mcsor_chains_rhs_argument_checks_before_setup():
    rp, ci, v = _lap1d(10)
    h = C.c_void_p()
    assert lib.pmg_mcsor_create_csr(10, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, C.byref(h)) == 0  # copies nothing to the device
    seeds = np.arange(4, dtype=np.uint64)
    B, Y = C.c_void_p(0x1000), C.c_void_p(0x2000)  # never dereferenced: every call below fails its checks first
    out = C.c_uint64()
    call = lib.pmg_mcsor_sample_chains_rhs
    assert call(h, 0, seeds.ctypes.data, B, Y, 1, 1, 0, C.byref(out), None) == ARG_OUTOFRANGE
    assert call(h, -2, seeds.ctypes.data, B, Y, 1, 1, 0, C.byref(out), None) == ARG_OUTOFRANGE
    assert call(h, 4, None, B, Y, 1, 1, 0, C.byref(out), None) == ARG_NULL
    assert call(h, 4, seeds.ctypes.data, None, Y, 1, 1, 0, C.byref(out), None) == ARG_NULL
    assert call(h, 4, seeds.ctypes.data, B, None, 1, 1, 0, C.byref(out), None) == ARG_NULL
    assert call(None, 4, seeds.ctypes.data, B, Y, 1, 1, 0, C.byref(out), None) == ARG_NULL
    assert call(h, 4, seeds.ctypes.data, B, Y, 1, 1, 0, C.byref(out), None) == ARG_WRONGSTATE
    assert b"pmg_mcsor_setup" in lib.pmg_last_error_string()
    assert lib.pmg_mcsor_destroy(C.byref(h)) == 0


def _hierarchy_handle():
    """a two-level caller-supplied hierarchy, not set up (set-up would factor on the device)"""
    rp, ci, v = _lap1d(8)
    rpc, cic, vc = _lap1d(4)
    prp = np.arange(9, dtype=np.int32)
    pci = (np.arange(8) // 2).astype(np.int32)
    pv = np.ones(8)
    keep = (rp, ci, v, rpc, cic, vc, prp, pci, pv)
    h = C.c_void_p()
    assert lib.pmg_mgmc_create_hierarchy(2, C.byref(h)) == 0
    assert lib.pmg_mgmc_set_level_operator(h, 0, 4, rpc.ctypes.data, cic.ctypes.data, vc.ctypes.data) == 0
    assert lib.pmg_mgmc_set_level_operator(h, 1, 8, rp.ctypes.data, ci.ctypes.data, v.ctypes.data) == 0
    assert lib.pmg_mgmc_set_level_interpolation(h, 1, 8, 4, prp.ctypes.data, pci.ctypes.data, pv.ctypes.data) == 0
    return h, keep


def _mg_call(h, nchains, seeds, B=C.c_void_p(0x1000), Y=C.c_void_p(0x2000)):
    out = C.c_uint64()
    return lib.pmg_mgmc_sample_chains_rhs(h, nchains, seeds, B, Y, 2, 0, 0, C.byref(out), None, None, None)


def test_mgmc_chains_rhs_argument_checks_before_setup():
    h, _keep = _hierarchy_handle()
    seeds = np.arange(3, dtype=np.uint64)
    assert _mg_call(h, 0, seeds.ctypes.data) == ARG_OUTOFRANGE
    assert _mg_call(h, 3, None) == ARG_NULL
    assert _mg_call(h, 3, seeds.ctypes.data, B=None) == ARG_NULL
    assert _mg_call(h, 3, seeds.ctypes.data, Y=None) == ARG_NULL
    assert _mg_call(None, 3, seeds.ctypes.data) == ARG_NULL
    assert _mg_call(h, 3, seeds.ctypes.data) == ARG_WRONGSTATE
    assert lib.pmg_mgmc_destroy(C.byref(h)) == 0


def test_woodbury_chains_reject_a_null_handle():
    seeds = np.arange(3, dtype=np.uint64)
    b, W = C.c_void_p(0x1000), C.c_void_p(0x2000)
    assert lib.pmg_woodbury_noisy_rhs_chains(None, 3, seeds.ctypes.data, 0, b, W, None) == ARG_NULL
    assert lib.pmg_woodbury_correct_chains(None, 3, W, None) == ARG_NULL


def _wb_create(n, k, B, ldb, S, out=True):
    h = C.c_void_p()
    st = lib.pmg_woodbury_create(n, k, B, ldb, S, None, C.byref(h) if out else None)
    assert st != 0 and not h.value  # every call here is refused: no handle comes back
    return st, h


def test_woodbury_create_rejects_bad_arguments_before_device_work():
    B = np.ones((4, 2), order="F")
    S = np.array([30.0, 40.0])
    Bp, Sp = B.ctypes.data, S.ctypes.data
    for k in (0, -1, 65):
        assert _wb_create(4, k, Bp, 4, Sp)[0] == ARG_OUTOFRANGE, k
        assert b"rank k" in lib.pmg_last_error_string()
    assert _wb_create(4, 2, Bp, 3, Sp)[0] == ARG_OUTOFRANGE  # ldb < n
    assert b"leading dimension 3" in lib.pmg_last_error_string()
    assert _wb_create(-1, 2, Bp, 4, Sp)[0] == ARG_OUTOFRANGE
    assert _wb_create(4, 2, None, 4, Sp)[0] == ARG_NULL  # null B with n > 0
    assert _wb_create(4, 2, Bp, 4, None)[0] == ARG_NULL
    assert _wb_create(4, 2, Bp, 4, Sp, out=False)[0] == ARG_NULL
    assert _wb_create(0, 2, None, 0, None)[0] == ARG_NULL  # n = 0 may come without B, not without S


def test_woodbury_calls_reject_a_null_handle():
    p, q = C.c_void_p(0x1000), C.c_void_p(0x2000)
    bc, cc = C.c_void_p(), C.c_void_p()
    assert lib.pmg_woodbury_column(None, 0, C.byref(bc), C.byref(cc), None) == ARG_NULL
    assert lib.pmg_woodbury_set_c_column(None, 0, p, None) == ARG_NULL
    assert lib.pmg_woodbury_finish(None) == ARG_NULL
    assert lib.pmg_woodbury_noisy_rhs(None, p, q, 1, 2, None) == ARG_NULL
    assert lib.pmg_woodbury_correct(None, p, None) == ARG_NULL
    assert lib.pmg_woodbury_get_correction(None, p) == ARG_NULL
    h = C.c_void_p()
    assert lib.pmg_woodbury_destroy(C.byref(h)) == 0 and lib.pmg_woodbury_destroy(None) == 0
