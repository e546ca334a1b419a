"""The Rao-Blackwellised statistics group (pmg_rbstats_*) is declared, bound and exported, rejects bad calls and bad matrices
before any device work, and reports the conditional precisions of the header's host formula bit for bit.
CPU only: every call here returns before the device is touched."""
import ctypes as C

import numpy as np
import pytest

import rbstats_cases as R
from parmgmc_amd import capi
from parmgmc_amd.capi import lib

ARG_NULL, ARG_OUTOFRANGE, ARG_WRONGSTATE, ARG_SIZ, ARG_WRONG = 85, 63, 73, 60, 62
NEW = ["pmg_rbstats_create_csr", "pmg_rbstats_destroy", "pmg_rbstats_set_lowrank", "pmg_rbstats_set_rhs", "pmg_rbstats_set_stream", "pmg_rbstats_update", "pmg_rbstats_callback",
       "pmg_rbstats_sample_callback", "pmg_rbstats_cond_mean", "pmg_rbstats_reset", "pmg_rbstats_get_count", "pmg_rbstats_get_fields", "pmg_rbstats_get_cond_precision",
       "pmg_rbstats_get_algorithmic_bytes"]


def test_new_symbols_are_exported_and_declared():
    declared = capi.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi._sig, name
    import parmgmc_amd

    assert hasattr(parmgmc_amd, "RBStats")


def _create(rowptr, colidx, vals, nchains=4):
    rp, ci, v = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colidx, np.int32), np.ascontiguousarray(vals, np.float64)
    h = C.c_void_p()
    st = lib.pmg_rbstats_create_csr(len(rp) - 1, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, nchains, C.byref(h))
    return st, h


TRI = ([0, 2, 5, 7], [0, 1, 0, 1, 2, 1, 2], [2.0, -1.0, -1.0, 2.0, -1.0, -1.0, 2.0])  # tridiag(-1, 2, -1), 3 rows


def _handle(nchains=4):
    st, h = _create(*TRI, nchains=nchains)
    assert st == 0 and h.value  # allocates nothing on the device
    return h


def test_create_argument_checks():
    rp, ci, v = (np.ascontiguousarray(a, t) for a, t in zip(TRI, (np.int32, np.int32, np.float64)))
    h = C.c_void_p()
    assert lib.pmg_rbstats_create_csr(3, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 4, None) == ARG_NULL
    assert lib.pmg_rbstats_create_csr(0, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 4, C.byref(h)) == ARG_OUTOFRANGE
    assert lib.pmg_rbstats_create_csr(-3, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 4, C.byref(h)) == ARG_OUTOFRANGE
    assert lib.pmg_rbstats_create_csr(3, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 0, C.byref(h)) == ARG_OUTOFRANGE
    assert lib.pmg_rbstats_create_csr(3, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, -2, C.byref(h)) == ARG_OUTOFRANGE
    assert lib.pmg_rbstats_create_csr(3, None, ci.ctypes.data, v.ctypes.data, 4, C.byref(h)) == ARG_NULL
    assert lib.pmg_rbstats_create_csr(3, rp.ctypes.data, None, v.ctypes.data, 4, C.byref(h)) == ARG_NULL
    assert lib.pmg_rbstats_create_csr(3, rp.ctypes.data, ci.ctypes.data, None, 4, C.byref(h)) == ARG_NULL
    assert not h.value
    for nchains in (1, 64, 1000):
        assert lib.pmg_rbstats_create_csr(3, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, nchains, C.byref(h)) == 0 and h.value
        assert lib.pmg_rbstats_destroy(C.byref(h)) == 0 and not h.value
    assert lib.pmg_rbstats_destroy(C.byref(h)) == 0  # destroying NULL is a no-op
    assert lib.pmg_rbstats_destroy(None) == 0


@pytest.mark.parametrize(
    "why,rowptr,colidx,vals,code,text",
    [
        ("missing diagonal", [0, 2, 4, 6], [0, 1, 0, 2, 1, 2], [2.0, -1.0, -1.0, -1.0, -1.0, 2.0], ARG_WRONG, b"no stored diagonal"),
        ("zero diagonal", TRI[0], TRI[1], [2.0, -1.0, -1.0, 0.0, -1.0, -1.0, 2.0], ARG_WRONG, b"positive and finite"),
        ("negative diagonal", TRI[0], TRI[1], [2.0, -1.0, -1.0, 2.0, -1.0, -1.0, -2.0], ARG_WRONG, b"positive and finite"),
        ("NaN diagonal", TRI[0], TRI[1], [np.nan, -1.0, -1.0, 2.0, -1.0, -1.0, 2.0], ARG_WRONG, b"positive and finite"),
        ("infinite diagonal", TRI[0], TRI[1], [2.0, -1.0, -1.0, np.inf, -1.0, -1.0, 2.0], ARG_WRONG, b"positive and finite"),
        ("diagonal stored twice", [0, 3, 6, 8], [0, 1, 0, 0, 1, 2, 1, 2], [1.0, -1.0, 1.0, -1.0, 2.0, -1.0, -1.0, 2.0], ARG_WRONG, b"twice"),
        ("column out of range", TRI[0], [0, 1, 0, 1, 3, 1, 2], TRI[2], ARG_OUTOFRANGE, b"out of range"),
        ("negative column", TRI[0], [0, -1, 0, 1, 2, 1, 2], TRI[2], ARG_OUTOFRANGE, b"out of range"),
        ("rowptr not monotone", [0, 2, 1, 7], TRI[1], TRI[2], ARG_WRONG, b"monotone"),
    ],
)
def test_rejected_matrices(why, rowptr, colidx, vals, code, text):
    """the code pmg_mcsor_setup gives a row without a stored diagonal (PMG_ERR_ARG_WRONG) for every defect of the diagonal; its
    codes for the structural defects"""
    st, h = _create(rowptr, colidx, vals)
    assert st == code and not h.value, why
    assert text in lib.pmg_last_error_string(), (why, lib.pmg_last_error_string())


def test_missing_diagonal_has_the_code_of_mcsor_setup():
    rp, ci, v = np.array([0, 2, 4, 6], np.int32), np.array([0, 1, 0, 2, 1, 2], np.int32), np.array([2.0, -1.0, -1.0, -1.0, -1.0, 2.0])
    mc = C.c_void_p()
    assert lib.pmg_mcsor_create_csr(3, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, C.byref(mc)) == 0
    want = lib.pmg_mcsor_setup(mc)  # fails on its structural checks, before any device work
    assert want != 0
    assert lib.pmg_mcsor_destroy(C.byref(mc)) == 0
    st, h = _create(rp, ci, v)
    assert st == want and not h.value


def test_argument_checks_before_the_device():
    h = _handle()
    Y, M = C.c_void_p(0x2000), C.c_void_p(0x4000)  # never dereferenced: every call below fails its checks first
    B, S = np.asfortranarray(np.ones((3, 2))), np.ones(2)
    q = np.zeros(3)
    by = C.c_double()
    # set_lowrank
    assert lib.pmg_rbstats_set_lowrank(None, 2, B.ctypes.data, S.ctypes.data) == ARG_NULL
    assert lib.pmg_rbstats_set_lowrank(h, -1, B.ctypes.data, S.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_rbstats_set_lowrank(h, 65, B.ctypes.data, S.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_rbstats_set_lowrank(h, 2, None, S.ctypes.data) == ARG_NULL
    assert lib.pmg_rbstats_set_lowrank(h, 2, B.ctypes.data, None) == ARG_NULL
    assert lib.pmg_rbstats_set_lowrank(h, 2, B.ctypes.data, (-5.0 * S).ctypes.data) == ARG_WRONG  # q = 2 - 10 < 0
    assert lib.pmg_rbstats_get_cond_precision(h, q.ctypes.data) == 0 and np.array_equal(q, [2.0, 2.0, 2.0])  # the rejected term changed nothing
    assert lib.pmg_rbstats_set_lowrank(h, 2, B.ctypes.data, S.ctypes.data) == 0  # host copies only
    assert lib.pmg_rbstats_set_lowrank(h, 0, None, None) == 0
    # set_rhs, set_stream
    assert lib.pmg_rbstats_set_rhs(None, Y) == ARG_NULL
    assert lib.pmg_rbstats_set_rhs(h, Y) == 0 and lib.pmg_rbstats_set_rhs(h, None) == 0
    assert lib.pmg_rbstats_set_stream(None, None) == ARG_NULL
    assert lib.pmg_rbstats_set_stream(h, None) == 0
    # update, cond_mean and the callbacks
    assert lib.pmg_rbstats_update(None, Y, None) == ARG_NULL
    assert lib.pmg_rbstats_update(h, None, None) == ARG_NULL
    assert lib.pmg_rbstats_cond_mean(None, Y, M, None) == ARG_NULL
    assert lib.pmg_rbstats_cond_mean(h, None, M, None) == ARG_NULL
    assert lib.pmg_rbstats_cond_mean(h, Y, None, None) == ARG_NULL
    assert lib.pmg_rbstats_cond_mean(h, Y, Y, None) == ARG_WRONG  # in place
    assert lib.pmg_rbstats_callback(0, Y, 3, 4, None) == ARG_NULL
    assert lib.pmg_rbstats_callback(0, Y, 4, 4, h) == ARG_SIZ
    assert lib.pmg_rbstats_callback(0, Y, 3, 3, h) == ARG_SIZ
    assert lib.pmg_rbstats_callback(0, None, 3, 4, h) == ARG_NULL
    assert lib.pmg_rbstats_sample_callback(0, Y, 3, h) == ARG_SIZ  # a handle of 4 chains on a single-chain sampler
    assert lib.pmg_rbstats_sample_callback(0, Y, 3, None) == ARG_NULL
    # nothing recorded yet
    st, sm = C.c_int32(-1), C.c_int64(-1)
    assert lib.pmg_rbstats_get_count(None, C.byref(st), C.byref(sm)) == ARG_NULL
    assert lib.pmg_rbstats_get_count(h, C.byref(st), C.byref(sm)) == 0 and (st.value, sm.value) == (0, 0)
    assert lib.pmg_rbstats_get_count(h, None, None) == 0
    assert lib.pmg_rbstats_reset(None) == ARG_NULL
    assert lib.pmg_rbstats_reset(h) == 0
    assert lib.pmg_rbstats_get_fields(None, Y, Y, None) == ARG_NULL
    assert lib.pmg_rbstats_get_fields(h, Y, Y, None) == ARG_WRONGSTATE  # src/ms.c:233
    assert b"at least 2 samples" in lib.pmg_last_error_string()
    assert lib.pmg_rbstats_get_cond_precision(None, q.ctypes.data) == ARG_NULL
    assert lib.pmg_rbstats_get_cond_precision(h, None) == ARG_NULL
    assert lib.pmg_rbstats_get_algorithmic_bytes(None, C.byref(by)) == ARG_NULL
    assert lib.pmg_rbstats_get_algorithmic_bytes(h, None) == ARG_NULL
    assert lib.pmg_rbstats_get_algorithmic_bytes(h, C.byref(by)) == 0 and by.value == 12 * 7 + 8 * 3 * 4 + 48 * 3
    assert lib.pmg_rbstats_destroy(C.byref(h)) == 0


@pytest.mark.parametrize("M", R.matrices() + R.integer_matrices() + [R.diagonal(33, 1)], ids=lambda M: M.name)
@pytest.mark.parametrize("k", R.RANKS)
def test_cond_precision_is_the_host_formula_bit_for_bit(M, k):
    st, h = _create(M.rowptr, M.colidx, M.vals, nchains=1)
    assert st == 0
    lr = R.lowrank(M.n, k, seed=M.n)
    if lr is not None:
        assert lib.pmg_rbstats_set_lowrank(h, k, lr[0].ctypes.data, lr[1].ctypes.data) == 0
    q = np.zeros(M.n)
    assert lib.pmg_rbstats_get_cond_precision(h, q.ctypes.data) == 0
    want = R.cond_precision_host(M, lr)
    assert np.array_equal(q, want)
    if lr is not None:
        base = R.cond_precision_host(M)
        assert (q >= base).all() and ((q > base).any() or M.n == 1) and q[M.n // 2] == base[M.n // 2]  # the term is there; not on B's zero row
        assert lib.pmg_rbstats_set_lowrank(h, 0, None, None) == 0  # and goes away
        assert lib.pmg_rbstats_get_cond_precision(h, q.ctypes.data) == 0
        assert np.array_equal(q, R.cond_precision_host(M))
    assert lib.pmg_rbstats_destroy(C.byref(h)) == 0


def test_python_wrapper_refuses_rb_with_callback():
    """rb= together with callback= is a ValueError, raised before anything reaches the library"""
    from parmgmc_amd import MGMC
    from parmgmc_amd.wrappers import WoodburySampler

    class _Y:  # stands for a tensor: the check comes first
        pass

    mg = MGMC.__new__(MGMC)
    mg._h, mg.n = None, 8
    with pytest.raises(ValueError):
        mg.sample(_Y(), _Y(), 1, 0, callback=lambda it, y: None, rb=object())
    wb = WoodburySampler.__new__(WoodburySampler)
    wb._h = None
    with pytest.raises(ValueError):
        wb.run_chains(_Y(), _Y(), 1, [0], callback=lambda it, y: None, rb=object())
