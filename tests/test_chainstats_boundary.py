"""The chain-statistics group (pmg_chainstats_*, pmg_gelman_rubin) is declared, bound and exported, rejects bad calls
before any device work, and pmg_gelman_rubin is GelmanRubin of the reference's examples/ex7.c:61-93 term by term.
CPU only: every call here returns before the device is touched."""
import ctypes as C

import numpy as np
import pytest

from parmgmc_amd import capi
from parmgmc_amd.capi import lib

ARG_NULL, ARG_OUTOFRANGE, ARG_WRONGSTATE, ARG_SIZ = 85, 63, 73, 60
MAX_QOI = 4
NEW = ["pmg_chainstats_create", "pmg_chainstats_destroy", "pmg_chainstats_set_qoi", "pmg_chainstats_set_stream", "pmg_chainstats_update", "pmg_chainstats_callback",
       "pmg_chainstats_sample_callback", "pmg_chainstats_reset", "pmg_chainstats_get_count", "pmg_chainstats_get_fields", "pmg_chainstats_get_trace", "pmg_gelman_rubin",
       "pmg_chainstats_rhat"]
EPS = np.finfo(np.float64).eps


def test_new_symbols_are_exported_and_declared():
    declared = capi.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi._sig, name
    import parmgmc_amd

    assert hasattr(parmgmc_amd, "ChainStats") and hasattr(parmgmc_amd, "gelman_rubin")


def _handle(n=10, nchains=4, nqoi=2, max_steps=3):
    h = C.c_void_p()
    assert lib.pmg_chainstats_create(n, nchains, nqoi, max_steps, C.byref(h)) == 0  # allocates nothing on the device
    return h


def test_create_argument_checks():
    h = C.c_void_p()
    assert lib.pmg_chainstats_create(10, 4, 1, 5, None) == ARG_NULL
    assert lib.pmg_chainstats_create(0, 4, 1, 5, C.byref(h)) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_create(10, 0, 1, 5, C.byref(h)) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_create(10, -2, 1, 5, C.byref(h)) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_create(10, 4, -1, 5, C.byref(h)) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_create(10, 4, MAX_QOI + 1, 5, C.byref(h)) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_create(10, 4, 1, 0, C.byref(h)) == ARG_OUTOFRANGE
    assert not h.value
    for nchains, nqoi in ((1, 0), (1, MAX_QOI), (1000, 1)):
        assert lib.pmg_chainstats_create(10, nchains, nqoi, 1, C.byref(h)) == 0 and h.value
        assert lib.pmg_chainstats_destroy(C.byref(h)) == 0 and not h.value
    assert lib.pmg_chainstats_destroy(C.byref(h)) == 0  # destroying NULL is a no-op


def test_argument_checks_before_the_device():
    h = _handle()
    Y = C.c_void_p(0x2000)  # never dereferenced: every call below fails its checks first
    w = np.ones(10)
    vals = np.zeros(64)
    gr = C.c_double()
    # set_qoi
    assert lib.pmg_chainstats_set_qoi(None, 0, w.ctypes.data) == ARG_NULL
    assert lib.pmg_chainstats_set_qoi(h, -1, w.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_set_qoi(h, 2, w.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_set_qoi(h, 0, w.ctypes.data) == 0  # host copy only
    assert lib.pmg_chainstats_set_qoi(h, 0, None) == 0  # back to all ones
    # update and the callbacks
    assert lib.pmg_chainstats_update(None, Y, None) == ARG_NULL
    assert lib.pmg_chainstats_update(h, None, None) == ARG_NULL
    assert lib.pmg_chainstats_callback(0, Y, 10, 4, None) == ARG_NULL
    assert lib.pmg_chainstats_callback(0, Y, 11, 4, h) == ARG_SIZ
    assert lib.pmg_chainstats_callback(0, Y, 10, 3, h) == ARG_SIZ
    assert lib.pmg_chainstats_callback(0, None, 10, 4, h) == ARG_NULL
    assert lib.pmg_chainstats_sample_callback(0, Y, 10, h) == ARG_SIZ  # a handle of 4 chains on a single-chain sampler
    assert lib.pmg_chainstats_set_stream(None, None) == ARG_NULL
    assert lib.pmg_chainstats_set_stream(h, None) == 0
    # nothing recorded yet
    st, sm = C.c_int32(-1), C.c_int64(-1)
    assert lib.pmg_chainstats_get_count(None, C.byref(st), C.byref(sm)) == ARG_NULL
    assert lib.pmg_chainstats_get_count(h, C.byref(st), C.byref(sm)) == 0 and (st.value, sm.value) == (0, 0)
    assert lib.pmg_chainstats_reset(None) == ARG_NULL
    assert lib.pmg_chainstats_reset(h) == 0
    assert lib.pmg_chainstats_get_fields(None, Y, Y, None) == ARG_NULL
    assert lib.pmg_chainstats_get_fields(h, Y, Y, None) == ARG_WRONGSTATE  # src/ms.c:233
    assert b"at least 2 samples" in lib.pmg_last_error_string()
    # windows
    assert lib.pmg_chainstats_get_trace(None, 0, 0, 0, vals.ctypes.data) == ARG_NULL
    assert lib.pmg_chainstats_get_trace(h, 2, 0, 0, vals.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_get_trace(h, -1, 0, 0, vals.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_get_trace(h, 0, 0, 1, vals.ctypes.data) == ARG_OUTOFRANGE  # nothing recorded
    assert lib.pmg_chainstats_get_trace(h, 0, -1, 0, vals.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_get_trace(h, 0, 0, -1, vals.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_get_trace(h, 0, 1, 0, vals.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_get_trace(h, 0, 0, 0, vals.ctypes.data) == 0  # the empty window
    assert lib.pmg_chainstats_rhat(None, 0, 0, 2, C.byref(gr)) == ARG_NULL
    assert lib.pmg_chainstats_rhat(h, 0, 0, 2, C.byref(gr)) == ARG_OUTOFRANGE  # window beyond the record
    assert lib.pmg_chainstats_rhat(h, 0, 0, 0, C.byref(gr)) == ARG_OUTOFRANGE  # fewer than 2 steps
    assert lib.pmg_chainstats_rhat(h, 3, 0, 0, C.byref(gr)) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_destroy(C.byref(h)) == 0
    # a handle without QOI has no trace; one chain has no R-hat
    h = _handle(nqoi=0)
    assert lib.pmg_chainstats_get_trace(h, 0, 0, 0, vals.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_set_qoi(h, 0, None) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_destroy(C.byref(h)) == 0
    h = _handle(nchains=1, nqoi=1)
    assert lib.pmg_chainstats_rhat(h, 0, 0, 0, C.byref(gr)) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_destroy(C.byref(h)) == 0


def test_gelman_rubin_argument_checks():
    v = np.arange(6.0)
    gr = C.c_double()
    assert lib.pmg_gelman_rubin(1, 6, v.ctypes.data, C.byref(gr)) == ARG_OUTOFRANGE
    assert lib.pmg_gelman_rubin(6, 1, v.ctypes.data, C.byref(gr)) == ARG_OUTOFRANGE
    assert lib.pmg_gelman_rubin(2, 3, None, C.byref(gr)) == ARG_NULL
    assert lib.pmg_gelman_rubin(2, 3, v.ctypes.data, None) == ARG_NULL


def gelman_rubin_ref(vals):
    """examples/ex7.c:61-93 restated: the same terms in the same order, one rounding per operation"""
    vals = np.asarray(vals, np.float64)
    chains, n = vals.shape
    fn, fc = np.float64(n), np.float64(chains)
    one = np.float64(1.0)
    means = np.zeros(chains)
    for i in range(chains):
        for j in range(n):
            means[i] += one / fn * vals[i, j]
    mean = np.float64(0.0)
    for i in range(chains):
        mean += one / fc * means[i]
    B = np.float64(0.0)
    for i in range(chains):
        B += fn / (fc - one) * (means[i] - mean) * (means[i] - mean)
    vars_ = np.zeros(chains)
    for i in range(chains):
        for j in range(n):
            vars_[i] += one / (fn - one) * (vals[i, j] - means[i]) * (vals[i, j] - means[i])
    W = np.float64(0.0)
    for i in range(chains):
        W += one / fc * vars_[i]
    return ((fn - one) / fn * W + one / fn * B) / W


def _gr(vals):
    v = np.ascontiguousarray(vals, np.float64)
    gr = C.c_double()
    assert lib.pmg_gelman_rubin(v.shape[0], v.shape[1], v.ctypes.data, C.byref(gr)) == 0
    return gr.value


@pytest.mark.parametrize("chains", [2, 8])
@pytest.mark.parametrize("n", [2, 50, 1000])
def test_gelman_rubin_random_traces(chains, n):
    rng = np.random.default_rng(1000 * chains + n)
    tol = 8 * chains * n * EPS
    for offset, spread in ((0.0, 0.0), (3.0, 0.5), (-40.0, 2.0)):
        vals = offset + rng.standard_normal((chains, n)) + spread * rng.standard_normal((chains, 1))
        want = gelman_rubin_ref(vals)
        got = _gr(vals)
        assert abs(got - want) <= tol * abs(want), (got, want)


def test_gelman_rubin_hand_computed():
    # chains (1, 2, 3) and (2, 4, 9): means 2 and 5, total mean 3.5, B = 3 / 1 * (2.25 + 2.25) = 13.5,
    # variances (1 + 0 + 1) / 2 = 1 and (9 + 1 + 16) / 2 = 13, W = 7, R = (2/3 * 7 + 1/3 * 13.5) / 7 = 55 / 42
    got = _gr([[1.0, 2.0, 3.0], [2.0, 4.0, 9.0]])
    assert abs(got - 55.0 / 42.0) <= 8 * 2 * 3 * EPS * (55.0 / 42.0), got


@pytest.mark.parametrize("chains", [2, 8])
@pytest.mark.parametrize("n", [2, 50, 1000])
def test_gelman_rubin_identical_chains(chains, n):
    """B = 0 up to rounding: R = (n - 1) / n"""
    rng = np.random.default_rng(7 + n)
    row = rng.standard_normal(n)
    got = _gr(np.tile(row, (chains, 1)))
    want = (n - 1.0) / n
    assert abs(got - want) <= 8 * chains * n * EPS * want, (got, want)


def test_python_wrapper_refuses_stats_with_callback():
    """stats= together with callback= is a ValueError, raised before anything reaches the library"""
    from parmgmc_amd import MGMC
    from parmgmc_amd.wrappers import WoodburySampler

    class _Y:  # stands for a tensor: the check comes first
        pass

    mg = MGMC.__new__(MGMC)
    mg._h, mg.n = None, 8
    with pytest.raises(ValueError):
        mg.sample(_Y(), _Y(), 1, 0, callback=lambda it, y: None, stats=object())
    wb = WoodburySampler.__new__(WoodburySampler)
    wb._h = None
    with pytest.raises(ValueError):
        wb.run_chains(_Y(), _Y(), 1, [0], callback=lambda it, y: None, stats=object())
