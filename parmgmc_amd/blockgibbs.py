"""Coloured block Gibbs sampler (pmg_blockgibbs_*): the Python mirror, as the classes of wrappers.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi, wrappers
from .capi import check, lib
from .wrappers import _blocks, _chains, _per_chain_rhs, _ptr, _stream, _update_all


class BlockGibbs:
    """Coloured block Gibbs sampler: the multiplicative patch smoother of the reference's examples/ex13.py:11-22 (PCASM
    multiplicative, every patch a cholsampler).  blocks: a sequence of row lists (caller's order, may overlap)."""

    def __init__(self, rowptr, colidx, vals, blocks, block_colors=None, layout=None):
        """block_colors: a colour per block instead of first-fit.  layout = (ld, pos_of_row): vectors indexed by position"""
        self._rowptr = np.ascontiguousarray(rowptr, np.int32)
        self._colidx = np.ascontiguousarray(colidx, np.int32)
        self._vals = np.ascontiguousarray(vals, np.float64)
        self.n = len(self._rowptr) - 1
        self.len = self.n if layout is None else int(layout[0])  # entries of a vector: rows, or positions of the layout
        self.nblocks, bp, br = _blocks(blocks)
        self._h = C.c_void_p()
        check(lib.pmg_blockgibbs_create_csr(self.n, self._rowptr.ctypes.data, self._colidx.ctypes.data, self._vals.ctypes.data, self.nblocks, bp.ctypes.data, br.ctypes.data, C.byref(self._h)))
        try:
            if block_colors is not None:
                bc = np.ascontiguousarray(block_colors, np.int32)
                assert len(bc) == self.nblocks
                check(lib.pmg_blockgibbs_set_coloring(self._h, int(bc.max()) + 1 if len(bc) else 0, bc.ctypes.data))
            if layout is not None:
                ld, pos = layout
                pos = np.ascontiguousarray(pos, np.int32)
                assert len(pos) == self.n
                check(lib.pmg_blockgibbs_set_layout(self._h, int(ld), pos.ctypes.data))
        except Exception:
            self.destroy()
            raise

    def setup(self):
        check(lib.pmg_blockgibbs_setup(self._h))
        return self

    def set_sweep_type(self, t: int):
        check(lib.pmg_blockgibbs_set_sweep_type(self._h, t))

    def get_sweep_type(self) -> int:
        t = C.c_int()
        check(lib.pmg_blockgibbs_get_sweep_type(self._h, C.byref(t)))
        return t.value

    def get_num_colors(self) -> int:
        n = C.c_int32()
        check(lib.pmg_blockgibbs_get_num_colors(self._h, C.byref(n)))
        return n.value

    def get_coloring(self) -> np.ndarray:
        out = np.zeros(max(self.nblocks, 1), np.int32)
        check(lib.pmg_blockgibbs_get_coloring(self._h, out.ctypes.data))
        return out[: self.nblocks]

    def get_num_slots(self) -> int:
        n = C.c_int32()
        check(lib.pmg_blockgibbs_get_num_slots(self._h, C.byref(n)))
        return n.value

    def block_factor(self, p: int) -> np.ndarray:
        """W_p = L_p^-1, (m, m)"""
        m = C.c_int32()
        check(lib.pmg_blockgibbs_get_block_factor(self._h, p, C.byref(m), None))
        W = np.zeros((m.value, m.value))
        check(lib.pmg_blockgibbs_get_block_factor(self._h, p, C.byref(m), W.ctypes.data))
        return W

    def apply(self, b, y):
        check(lib.pmg_blockgibbs_apply(self._h, _ptr(b), _ptr(y), _stream()))

    def sample(self, b, y, its: int, seed: int, counter0: int = 0) -> int:
        out = C.c_uint64()
        check(lib.pmg_blockgibbs_sample(self._h, _ptr(b), _ptr(y), its, seed, counter0, C.byref(out), _stream()))
        return out.value

    def sweep_xi(self, xi_slots, b, y, backward: bool = False):
        """one directional sweep with the normals of the slots read from xi_slots (nslots)"""
        check(lib.pmg_blockgibbs_sweep_xi(self._h, int(backward), _ptr(xi_slots), _ptr(b), _ptr(y), _stream()))

    def algorithmic_bytes(self) -> float:
        out = C.c_double()
        check(lib.pmg_blockgibbs_get_algorithmic_bytes(self._h, C.byref(out)))
        return out.value

    # --- many chains per call: Y is a contiguous (len, C) float64 tensor, len = n or the layout's ld ---
    def apply_chains(self, b, Y):
        """the deterministic sweep on every column of Y (= apply per column); b: one vector (len,) shared by the chains"""
        p, nc = _chains(Y, self.len)
        check(lib.pmg_blockgibbs_apply_chains(self._h, nc, _ptr(b), p, _stream()))

    def sample_chains(self, b, Y, its: int, seeds, counter0: int = 0, callback=None, stats=None, rb=None) -> int:
        """`its` samples of C chains; column c equals sample(b or b[:, c], Y[:, c], its, seeds[c], counter0) bit for bit.  b: one
        vector (len,) shared by the chains, or one right-hand side per chain (len, C).  callback(it, Y) after every sample; a
        raised exception aborts the loop.  stats: a ChainStats(len, C), rb: an RBStats of len rows and C chains, updated after
        every sample by the library's own callback (no Python in the loop; both exclude callback); both together are updated by
        one Python-level callback."""
        p, nc = _chains(Y, self.len)
        s = wrappers._seeds(seeds, nc)
        out = C.c_uint64()
        cb, ctx = None, None
        consumers = [x for x in (stats, rb) if x is not None]
        if consumers and callback is not None:
            raise ValueError("stats= / rb= and callback= exclude each other")
        if len(consumers) > 1:
            callback = _update_all(self.len, nc, *consumers)
        elif stats is not None:
            cb, ctx = stats._as_callback(self.len, nc, lib.pmg_chainstats_callback)
        elif rb is not None:
            cb, ctx = rb._as_callback(self.len, nc, lib.pmg_rbstats_callback)
        if callback is not None:

            def _cb(it, ptr, n, nchains, _ctx):
                try:
                    rc = callback(it, Y)
                    return int(rc) if rc else 0
                except Exception:  # pragma: no cover
                    import traceback

                    traceback.print_exc()
                    return 77

            cb = capi.CHAINS_CALLBACK(_cb)
        fn = lib.pmg_blockgibbs_sample_chains_rhs if _per_chain_rhs(b, self.len, nc) else lib.pmg_blockgibbs_sample_chains
        check(fn(self._h, nc, s.ctypes.data, _ptr(b), p, its, counter0, C.byref(out), cb, ctx, _stream()))
        return out.value

    def sweep_xi_chains(self, xi_slots, b, Y, backward: bool = False):
        """one directional sweep of every chain with the normals read from xi_slots (nslots, C)"""
        p, nc = _chains(Y, self.len)
        assert xi_slots.dim() == 2 and xi_slots.shape[1] == nc, f"need xi_slots of shape (nslots, {nc})"
        check(lib.pmg_blockgibbs_sweep_xi_chains(self._h, nc, int(backward), _ptr(xi_slots), _ptr(b), p, _stream()))

    def algorithmic_bytes_chains(self, nchains: int, per_chain_rhs: bool = False) -> float:
        """bytes of one noisy directional sweep of `nchains` chains, shared operands counted once"""
        out = C.c_double()
        check(lib.pmg_blockgibbs_get_algorithmic_bytes_chains(self._h, nchains, int(per_chain_rhs), C.byref(out)))
        return out.value

    def destroy(self):
        if self._h:
            check(lib.pmg_blockgibbs_destroy(C.byref(self._h)))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
