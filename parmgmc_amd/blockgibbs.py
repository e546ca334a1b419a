"""Coloured block Gibbs sampler (pmg_blockgibbs_*): the Python mirror, as the classes of wrappers.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .capi import check, lib
from .wrappers import _blocks, _ptr, _stream


class BlockGibbs:
    """Coloured block Gibbs sampler: the multiplicative patch smoother of the reference's examples/ex13.py:11-22 (PCASM
    multiplicative, every patch a cholsampler).  blocks: a sequence of row lists (caller's order, may overlap)."""

    def __init__(self, rowptr, colidx, vals, blocks, block_colors=None, layout=None):
        """block_colors: a colour per block instead of first-fit.  layout = (ld, pos_of_row): vectors indexed by position"""
        self._rowptr = np.ascontiguousarray(rowptr, np.int32)
        self._colidx = np.ascontiguousarray(colidx, np.int32)
        self._vals = np.ascontiguousarray(vals, np.float64)
        self.n = len(self._rowptr) - 1
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

    def destroy(self):
        if self._h:
            check(lib.pmg_blockgibbs_destroy(C.byref(self._h)))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
