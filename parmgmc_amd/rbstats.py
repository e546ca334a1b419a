"""parmgmc_amd.RBStats, the Python mirror of pmg_rbstats (Rao-Blackwellised chain statistics on the device), re-exported by
wrappers.py beside ChainStats.  It is a module of its own because tests/handle_steps.py catalogues every device-vector method of
the classes defined in wrappers.py for tests/test_gpu_call_history.py; the call-history contract of this handle is checked by
tests/test_gpu_rbstats_history.py instead."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .capi import check, lib
from .wrappers import _ptr, _stream


class RBStats:
    """pmg_rbstats: Rao-Blackwellised marginal mean and variance of every row of x ~ N(Q^-1 b, Q^-1) over all steps x chains
    samples, from the conditional means m_i = (b_i - sum_{j != i} Q_ij y_j) / Q_ii of the samples: mean = mean of m,
    var = 1 / Q_ii + var of m.  The same fields as ChainStats.fields() with less Monte Carlo error, for one pass over the matrix
    per step.
      A: a scipy.sparse matrix, an object with rowptr / colidx / vals (the oracle's CSR) or a (rowptr, colidx, vals) triple;
      lowrank = (B, S): Q = A + B diag(S) B^T with B (n, k); b: the right-hand side, a device tensor of n entries kept alive
      here, or None for zero."""

    def __init__(self, A, nchains: int = 1, lowrank=None, b=None):
        if hasattr(A, "indptr"):
            A = A.tocsr()
            rowptr, colidx, vals = A.indptr, A.indices, A.data
        elif hasattr(A, "rowptr"):
            rowptr, colidx, vals = A.rowptr, A.colidx, A.vals
        else:
            rowptr, colidx, vals = A
        rp, ci, v = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colidx, np.int32), np.ascontiguousarray(vals, np.float64)
        self.n, self.nchains, self.k = len(rp) - 1, int(nchains), 0
        self._h = C.c_void_p()
        self._b = None
        check(lib.pmg_rbstats_create_csr(self.n, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, self.nchains, C.byref(self._h)))
        if lowrank is not None:
            self.set_lowrank(*lowrank)
        self.set_rhs(b)

    @classmethod
    def dmda(cls, nx: int, ny: int, nz: int, kappa: float, nchains: int = 1, lowrank=None, b=None):
        """pmg_rbstats_create_dmda: the same statistics on the grid operator of Grid / MGMC(nx, ny, nz, kappa), matrix-free, with
        the bits of RBStats(oracle.shifted_laplace(nx, ny, nz, kappa)).  Rows in DMDA natural order (i fastest); lowrank = (B, S)
        with B (n, k) in natural numbering (pmg_make_observation_mats_dmda); b as for the constructor."""
        self = cls.__new__(cls)
        self.n, self.nchains, self.k = int(nx) * int(ny) * int(nz), int(nchains), 0
        self._h = C.c_void_p()
        self._b = None
        check(lib.pmg_rbstats_create_dmda(int(nx), int(ny), int(nz), float(kappa), self.nchains, C.byref(self._h)))
        if lowrank is not None:
            self.set_lowrank(*lowrank)
        self.set_rhs(b)
        return self

    def set_lowrank(self, B=None, S=None):
        """Q = A + B diag(S) B^T; B = None removes the term.  Forgets the recorded statistics."""
        if B is None:
            check(lib.pmg_rbstats_set_lowrank(self._h, 0, None, None))
            self.k = 0
            return
        B, S = np.asfortranarray(B, np.float64), np.ascontiguousarray(S, np.float64)
        assert B.shape == (self.n, len(S)), f"need B of shape ({self.n}, k) and k entries of S"
        check(lib.pmg_rbstats_set_lowrank(self._h, B.shape[1], B.ctypes.data, S.ctypes.data))
        self.k = B.shape[1]

    def set_rhs(self, b=None):
        """b: a contiguous float64 CUDA tensor of n entries (kept alive by this object), or None for zero"""
        assert b is None or b.numel() == self.n, f"need {self.n} entries"
        check(lib.pmg_rbstats_set_rhs(self._h, None if b is None else _ptr(b)))
        self._b = b

    def _check_sizes(self, n: int, nchains: int):
        assert (n, nchains) == (self.n, self.nchains), f"RBStats of {self.n} x {self.nchains} on samples of {n} x {nchains}"

    def update(self, Y):
        """one step: Y is a contiguous (n, C) float64 CUDA tensor (or (n,) for one chain), on the current stream"""
        assert Y.numel() == self.n * self.nchains and (Y.dim() == 1 or tuple(Y.shape) == (self.n, self.nchains)), f"need an ({self.n}, {self.nchains}) tensor"
        check(lib.pmg_rbstats_update(self._h, _ptr(Y), _stream()))

    def cond_mean(self, Y):
        """the conditional means of one step's samples as a tensor of Y's shape; records nothing"""
        import torch

        assert Y.numel() == self.n * self.nchains and (Y.dim() == 1 or tuple(Y.shape) == (self.n, self.nchains)), f"need an ({self.n}, {self.nchains}) tensor"
        M = torch.empty_like(Y)
        check(lib.pmg_rbstats_cond_mean(self._h, _ptr(Y), _ptr(M), _stream()))
        return M

    def _as_callback(self, n: int, nchains: int, fn):
        """(function pointer, context) for a sampler's callback argument; the callback launches on the current stream"""
        self._check_sizes(n, nchains)
        check(lib.pmg_rbstats_set_stream(self._h, _stream()))
        return C.cast(fn, C.c_void_p), self._h

    def reset(self):
        check(lib.pmg_rbstats_reset(self._h))

    def count(self):
        """(steps, samples = steps * chains)"""
        st, sm = C.c_int32(), C.c_int64()
        check(lib.pmg_rbstats_get_count(self._h, C.byref(st), C.byref(sm)))
        return st.value, sm.value

    def fields(self):
        """(mean, var): device tensors of n entries; var = 1 / Q_ii + the unbiased variance of m over all samples seen"""
        import torch

        mean = torch.empty(self.n, dtype=torch.float64, device="cuda")
        var = torch.empty(self.n, dtype=torch.float64, device="cuda")
        check(lib.pmg_rbstats_get_fields(self._h, _ptr(mean), _ptr(var), _stream()))
        return mean, var

    def cond_precision(self) -> np.ndarray:
        """q_i = Q_ii as a host array"""
        q = np.empty(self.n)
        check(lib.pmg_rbstats_get_cond_precision(self._h, q.ctypes.data))
        return q

    def algorithmic_bytes(self) -> float:
        out = C.c_double()
        check(lib.pmg_rbstats_get_algorithmic_bytes(self._h, C.byref(out)))
        return out.value

    def destroy(self):
        if self._h:
            check(lib.pmg_rbstats_destroy(C.byref(self._h)))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
