"""The multi-chain entry points of the coloured block Gibbs sampler (pmg_blockgibbs_apply_chains, _sample_chains,
_sample_chains_rhs, _sweep_xi_chains, _get_algorithmic_bytes_chains) are exported, declared and prototyped, and reject bad calls
before any device work, in the documented precedence: NULL arguments, ranges, sizes, state.
CPU only: every call here returns before the device is touched."""
import ctypes as C

import numpy as np

from parmgmc_amd import capi
from parmgmc_amd.capi import lib
from test_chains_boundary import _lap1d

ARG_NULL, ARG_OUTOFRANGE, ARG_WRONGSTATE = 85, 63, 73
NEW = ["pmg_blockgibbs_apply_chains", "pmg_blockgibbs_sample_chains", "pmg_blockgibbs_sample_chains_rhs", "pmg_blockgibbs_sweep_xi_chains", "pmg_blockgibbs_get_algorithmic_bytes_chains"]
B, Y, XI = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x3000)  # never dereferenced: every call below fails its checks first


def test_new_symbols_are_exported_declared_and_prototyped():
    declared = capi.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi._sig, name
    assert len(capi._sig["pmg_blockgibbs_sample_chains"][1]) == 11 and len(capi._sig["pmg_blockgibbs_sample_chains_rhs"][1]) == 11
    assert len(capi._sig["pmg_blockgibbs_apply_chains"][1]) == 5 and len(capi._sig["pmg_blockgibbs_sweep_xi_chains"][1]) == 7
    assert len(capi._sig["pmg_blockgibbs_get_algorithmic_bytes_chains"][1]) == 4


def _handle(n=10):
    """a tridiagonal operator with blocks of two rows; created, not set up (set-up uploads)"""
    rp, ci, v = _lap1d(n)
    bp = np.arange(0, n + 1, 2, dtype=np.int32)
    br = np.arange(n, dtype=np.int32)
    h = C.c_void_p()
    assert lib.pmg_blockgibbs_create_csr(n, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, len(bp) - 1, bp.ctypes.data, br.ctypes.data, C.byref(h)) == 0
    return h, (rp, ci, v, bp, br)


def _sample(fn, h, nchains, seeds, b=B, y=Y, its=1):
    out = C.c_uint64()
    return fn(h, nchains, seeds, b, y, its, 0, C.byref(out), None, None, None)


def test_argument_checks_before_setup_in_their_precedence():
    h, _keep = _handle()
    seeds = np.arange(4, dtype=np.uint64)
    sp = seeds.ctypes.data
    for fn in (lib.pmg_blockgibbs_sample_chains, lib.pmg_blockgibbs_sample_chains_rhs):
        # 1. NULL handle, seeds, b, Y -- also when the ranges are wrong as well
        assert _sample(fn, None, 4, sp) == ARG_NULL
        assert _sample(fn, h, 4, None) == ARG_NULL
        assert _sample(fn, h, 4, sp, b=None) == ARG_NULL
        assert _sample(fn, h, 4, sp, y=None) == ARG_NULL
        assert _sample(fn, h, 0, None) == ARG_NULL
        assert _sample(fn, h, 4, sp, y=None, its=-1) == ARG_NULL
        # 2. nchains < 1, its < 0 -- before the state
        assert _sample(fn, h, 0, sp) == ARG_OUTOFRANGE
        assert _sample(fn, h, -3, sp) == ARG_OUTOFRANGE
        assert _sample(fn, h, 4, sp, its=-1) == ARG_OUTOFRANGE
        # 3. sizes: more chains than the launches index, more elements than 2^40
        assert _sample(fn, h, 64 * 65535 + 1, sp) == ARG_OUTOFRANGE
        # 4. a well-formed call on a handle that is not set up
        assert _sample(fn, h, 4, sp) == ARG_WRONGSTATE
        assert b"pmg_blockgibbs_setup" in lib.pmg_last_error_string()
    assert lib.pmg_blockgibbs_apply_chains(None, 4, B, Y, None) == ARG_NULL
    assert lib.pmg_blockgibbs_apply_chains(h, 4, None, Y, None) == ARG_NULL
    assert lib.pmg_blockgibbs_apply_chains(h, 0, B, None, None) == ARG_NULL
    assert lib.pmg_blockgibbs_apply_chains(h, 0, B, Y, None) == ARG_OUTOFRANGE
    assert lib.pmg_blockgibbs_apply_chains(h, 64 * 65535 + 1, B, Y, None) == ARG_OUTOFRANGE
    assert lib.pmg_blockgibbs_apply_chains(h, 4, B, Y, None) == ARG_WRONGSTATE
    assert b"pmg_blockgibbs_setup" in lib.pmg_last_error_string()
    assert lib.pmg_blockgibbs_sweep_xi_chains(None, 4, 0, XI, B, Y, None) == ARG_NULL
    assert lib.pmg_blockgibbs_sweep_xi_chains(h, 4, 0, None, B, Y, None) == ARG_NULL
    assert lib.pmg_blockgibbs_sweep_xi_chains(h, 4, 0, XI, None, Y, None) == ARG_NULL
    assert lib.pmg_blockgibbs_sweep_xi_chains(h, 0, 0, XI, B, None, None) == ARG_NULL
    assert lib.pmg_blockgibbs_sweep_xi_chains(h, 0, 1, XI, B, Y, None) == ARG_OUTOFRANGE
    assert lib.pmg_blockgibbs_sweep_xi_chains(h, 4, 1, XI, B, Y, None) == ARG_WRONGSTATE
    assert b"pmg_blockgibbs_setup" in lib.pmg_last_error_string()
    assert lib.pmg_blockgibbs_destroy(C.byref(h)) == 0


def test_size_check_uses_the_layout_length():
    """2^40 elements: the length that counts is ld after pmg_blockgibbs_set_layout, n before"""
    h, _keep = _handle()
    seeds = np.arange(4, dtype=np.uint64)
    # 10 rows: 2^21 chains pass the size check (the state check answers; the seeds are never read) ...
    assert _sample(lib.pmg_blockgibbs_sample_chains, h, 1 << 21, seeds.ctypes.data) == ARG_WRONGSTATE
    pos = np.arange(10, dtype=np.int32)
    assert lib.pmg_blockgibbs_set_layout(h, 1 << 30, pos.ctypes.data) == 0  # ... and with ld = 2^30, 2^10 chains are the limit
    assert _sample(lib.pmg_blockgibbs_sample_chains, h, 1 << 10, seeds.ctypes.data) == ARG_WRONGSTATE
    assert _sample(lib.pmg_blockgibbs_sample_chains, h, (1 << 10) + 1, seeds.ctypes.data) == ARG_OUTOFRANGE
    assert lib.pmg_blockgibbs_apply_chains(h, (1 << 10) + 1, B, Y, None) == ARG_OUTOFRANGE
    assert lib.pmg_blockgibbs_destroy(C.byref(h)) == 0


def test_bytes_chains_checks():
    h, _keep = _handle()
    out = C.c_double()
    assert lib.pmg_blockgibbs_get_algorithmic_bytes_chains(None, 3, 0, C.byref(out)) == ARG_NULL
    assert lib.pmg_blockgibbs_get_algorithmic_bytes_chains(h, 3, 0, None) == ARG_NULL
    assert lib.pmg_blockgibbs_get_algorithmic_bytes_chains(h, 0, 0, C.byref(out)) == ARG_OUTOFRANGE
    assert lib.pmg_blockgibbs_get_algorithmic_bytes_chains(h, 3, 0, C.byref(out)) == ARG_WRONGSTATE
    assert lib.pmg_blockgibbs_get_algorithmic_bytes_chains(h, 3, 1, C.byref(out)) == ARG_WRONGSTATE
    assert lib.pmg_blockgibbs_destroy(C.byref(h)) == 0
