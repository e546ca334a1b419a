"""Thin Python mirrors of the C-ABI objects, for tests and benchmarks.

Device vectors are torch CUDA tensors (float64); only their ``data_ptr()`` and the current HIP stream cross
the boundary.  The method names follow the reference API (include/parmgmc/mc_sor.h:21-30)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import check, lib


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    import torch

    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous(), "need a contiguous float64 CUDA tensor"
    return C.c_void_p(t.data_ptr())


def _chains(Y, n):
    """(pointer, C) of a contiguous (n, C) float64 CUDA tensor: the chains layout of the C-ABI, chain fastest"""
    assert Y.dim() == 2 and Y.shape[0] == n, f"need an (n, C) tensor with n = {n}"
    return _ptr(Y), int(Y.shape[1])


def _per_chain_rhs(b, n, nchains):
    """True for one right-hand side per chain ((n, C), chain fastest), False for one shared vector (n,)"""
    if b.dim() == 1:
        assert b.shape[0] == n, f"need b of shape ({n},) or ({n}, {nchains})"
        return False
    assert tuple(b.shape) == (n, nchains), f"need b of shape ({n},) or ({n}, {nchains})"
    return True


def _seeds(seeds, nchains):
    s = np.ascontiguousarray([int(v) & 0xFFFFFFFFFFFFFFFF for v in seeds], np.uint64)
    assert len(s) == nchains, f"{len(s)} seeds for {nchains} chains"
    return s


class MCSOR:
    """MCSOR on an assembled AIJ matrix (reference include/parmgmc/mc_sor.h:21-30)."""

    def __init__(self, rowptr, colidx, vals, coloring=capi.COLORING_GREEDY, user_colors=None, idx_width=32):
        """idx_width 64: the index arrays cross the boundary as 64-bit PetscInt (pmg_mcsor_create_csr_idx)"""
        it = np.int64 if idx_width == 64 else np.int32
        self._rowptr = np.ascontiguousarray(rowptr, it)
        self._colidx = np.ascontiguousarray(colidx, it)
        self._vals = np.ascontiguousarray(vals, np.float64)
        self.n = len(self._rowptr) - 1
        self._h = C.c_void_p()
        if idx_width == 32:
            check(lib.pmg_mcsor_create_csr(self.n, self._rowptr.ctypes.data, self._colidx.ctypes.data, self._vals.ctypes.data, C.byref(self._h)))
        else:
            check(lib.pmg_mcsor_create_csr_idx(self.n, self._rowptr.ctypes.data, self._colidx.ctypes.data, self._vals.ctypes.data, idx_width, C.byref(self._h)))
        uc = None
        if user_colors is not None:
            uc = np.ascontiguousarray(user_colors, np.int32)
            coloring = capi.COLORING_USER
        try:
            check(lib.pmg_mcsor_set_coloring(self._h, coloring, None if uc is None else uc.ctypes.data))
        except Exception:
            self.destroy()
            raise

    def setup(self):
        check(lib.pmg_mcsor_setup(self._h))
        return self

    def set_omega(self, omega: float):
        check(lib.pmg_mcsor_set_omega(self._h, omega))

    def set_sweep_type(self, t: int):
        check(lib.pmg_mcsor_set_sweep_type(self._h, t))

    def get_sweep_type(self) -> int:
        t = C.c_int()
        check(lib.pmg_mcsor_get_sweep_type(self._h, C.byref(t)))
        return t.value

    def get_num_colors(self) -> int:
        n = C.c_int32()
        check(lib.pmg_mcsor_get_num_colors(self._h, C.byref(n)))
        return n.value

    def get_coloring(self) -> np.ndarray:
        out = np.zeros(max(self.n, 1), np.int32)
        check(lib.pmg_mcsor_get_coloring(self._h, out.ctypes.data))
        return out[: self.n]

    def apply(self, b, y):
        check(lib.pmg_mcsor_apply(self._h, _ptr(b), _ptr(y), _stream()))

    def sample(self, b, y, its: int, seed: int, counter0: int = 0, scaled: bool = True) -> int:
        out = C.c_uint64()
        check(lib.pmg_mcsor_sample(self._h, _ptr(b), _ptr(y), its, int(scaled), seed, counter0, C.byref(out), _stream()))
        return out.value

    def residual(self, b, y, r):
        check(lib.pmg_mcsor_residual(self._h, _ptr(b), _ptr(y), _ptr(r), _stream()))

    # --- many chains per call: Y is a contiguous (n, C) float64 tensor, b one vector shared by all chains ---
    def apply_chains(self, b, Y):
        """the deterministic sweep on every column of Y (= apply per column)"""
        p, nc = _chains(Y, self.n)
        check(lib.pmg_mcsor_apply_chains(self._h, nc, _ptr(b), p, _stream()))

    def sample_chains(self, b, Y, its: int, seeds, counter0: int = 0, scaled: bool = True) -> int:
        """`its` samples of C chains; column c equals sample(b, Y[:, c], its, seeds[c], counter0, scaled) bit for bit.  b: one
        vector (n,) shared by the chains, or one right-hand side per chain (n, C), column c = b[:, c].  The C entry point has no
        callback: for running statistics call ChainStats.update(Y) between calls (sample_chains(b, Y, 1, seeds, counter0 + it))."""
        p, nc = _chains(Y, self.n)
        s = _seeds(seeds, nc)
        out = C.c_uint64()
        fn = lib.pmg_mcsor_sample_chains_rhs if _per_chain_rhs(b, self.n, nc) else lib.pmg_mcsor_sample_chains
        check(fn(self._h, nc, s.ctypes.data, _ptr(b), p, its, int(scaled), counter0, C.byref(out), _stream()))
        return out.value

    # --- storage layout and per-colour sweeps (building blocks of the row-block distributed sampler) ---
    def layout_len(self) -> int:
        n = C.c_int32()
        check(lib.pmg_mcsor_layout_len(self._h, C.byref(n)))
        return n.value

    def get_layout(self) -> np.ndarray:
        """position of every row in the library's storage layout"""
        out = np.zeros(max(self.n, 1), np.int32)
        check(lib.pmg_mcsor_get_layout(self._h, out.ctypes.data))
        return out[: self.n]

    def set_noise_row_offset(self, row0: int):
        check(lib.pmg_mcsor_set_noise_row_offset(self._h, row0))

    def sweep_color_layout(self, color: int, b_lay, y_lay, noisy: bool = True, scaled: bool = True, seed: int = 0, counter: int = 0):
        check(lib.pmg_mcsor_sweep_color_layout(self._h, color, int(noisy), int(scaled), seed, counter, _ptr(b_lay), _ptr(y_lay), _stream()))

    def set_lowrank(self, B, S):
        """MATLRC A + B diag(S) B^T: B (n x k), S (k) host arrays (reference src/mc_sor.c:572-595)."""
        B = np.asfortranarray(B, dtype=np.float64)
        S = np.ascontiguousarray(S, np.float64)
        check(lib.pmg_mcsor_set_lowrank(self._h, B.shape[1], B.ctypes.data, S.ctypes.data))

    def lowrank_sizes(self):
        """(k, rows, dense): rank of the update (0: none) and the rows its passes run over; dense False = the row-compact form"""
        k, rows, dense = C.c_int32(), C.c_int64(), C.c_int()
        check(lib.pmg_mcsor_lowrank_sizes(self._h, C.byref(k), C.byref(rows), C.byref(dense)))
        return k.value, rows.value, bool(dense.value)

    def destroy(self):
        if self._h:
            check(lib.pmg_mcsor_destroy(C.byref(self._h)))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class GridMCSOR:
    """Matrix-free MCSOR on a DMDA grid for the operator of MatAssembleShiftedLaplaceFD
    (reference src/problems.c:14-75); owns planes [kz0, kz0+nz) of nx*ny*nzg."""

    def __init__(self, nx, ny, nz=1, kappa=1.0, kz0=0, nz_owned=None):
        self.nx, self.ny, self.nzg = nx, ny, nz
        self.kz0, self.nz = kz0, (nz if nz_owned is None else nz_owned)
        self._h = C.c_void_p()
        check(lib.pmg_grid_create(nx, ny, nz, self.kz0, self.nz, kappa, C.byref(self._h)))
        n = C.c_int64()
        check(lib.pmg_grid_cvec_len(self._h, C.byref(n)))
        self.cvec_len = n.value
        self.n = nx * ny * self.nz

    def new_cvec(self):
        import torch

        return torch.zeros(self.cvec_len, dtype=torch.float64, device="cuda")

    def to_cvec(self, nat, out=None):
        out = self.new_cvec() if out is None else out
        check(lib.pmg_grid_to_cvec(self._h, _ptr(nat), _ptr(out), _stream()))
        return out

    def from_cvec(self, cvec, out=None):
        import torch

        out = torch.empty(self.n, dtype=torch.float64, device="cuda") if out is None else out
        check(lib.pmg_grid_from_cvec(self._h, _ptr(cvec), _ptr(out), _stream()))
        return out

    def set_omega(self, omega: float):
        check(lib.pmg_grid_set_omega(self._h, omega))

    def set_sweep_type(self, t: int):
        check(lib.pmg_grid_set_sweep_type(self._h, t))

    def get_sweep_type(self) -> int:
        t = C.c_int()
        check(lib.pmg_grid_get_sweep_type(self._h, C.byref(t)))
        return t.value

    def get_num_colors(self) -> int:
        n = C.c_int32()
        check(lib.pmg_grid_get_num_colors(self._h, C.byref(n)))
        return n.value

    def get_coloring(self) -> np.ndarray:
        out = np.zeros(self.n, np.int32)
        check(lib.pmg_grid_get_coloring(self._h, out.ctypes.data))
        return out

    def apply(self, b, y):
        check(lib.pmg_grid_apply(self._h, _ptr(b), _ptr(y), _stream()))

    def apply_cvec(self, b, y):
        check(lib.pmg_grid_apply_cvec(self._h, _ptr(b), _ptr(y), _stream()))

    def sample(self, b, y, its: int, seed: int, counter0: int = 0, scaled: bool = True) -> int:
        out = C.c_uint64()
        check(lib.pmg_grid_sample(self._h, _ptr(b), _ptr(y), its, int(scaled), seed, counter0, C.byref(out), _stream()))
        return out.value

    def sample_cvec(self, b, y, its: int, seed: int, counter0: int = 0, scaled: bool = True) -> int:
        out = C.c_uint64()
        check(lib.pmg_grid_sample_cvec(self._h, _ptr(b), _ptr(y), its, int(scaled), seed, counter0, C.byref(out), _stream()))
        return out.value

    def sweep_color_cvec(self, color: int, b, y, noisy: bool = False, scaled: bool = True, seed: int = 0, counter: int = 0):
        check(lib.pmg_grid_sweep_color_cvec(self._h, color, int(noisy), int(scaled), seed, counter, _ptr(b), _ptr(y), _stream()))

    def sweep_color_planes_cvec(self, color: int, kbegin: int, kcount: int, b, y, noisy: bool = False, scaled: bool = True, seed: int = 0, counter: int = 0):
        check(lib.pmg_grid_sweep_color_planes_cvec(self._h, color, kbegin, kcount, int(noisy), int(scaled), seed, counter, _ptr(b), _ptr(y), _stream()))

    def halo_plane(self, color: int, side: int):
        """(owned_offset, ghost_offset, count) in doubles inside a cvec."""
        a, b, n = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib.pmg_grid_halo_plane(self._h, color, side, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def set_lowrank(self, B, S):
        B = np.asfortranarray(B, dtype=np.float64)
        S = np.ascontiguousarray(S, np.float64)
        check(lib.pmg_grid_set_lowrank(self._h, B.shape[1], B.ctypes.data, S.ctypes.data))

    def lowrank_sizes(self):
        """(k, rows, dense) as MCSOR.lowrank_sizes"""
        k, rows, dense = C.c_int32(), C.c_int64(), C.c_int()
        check(lib.pmg_grid_lowrank_sizes(self._h, C.byref(k), C.byref(rows), C.byref(dense)))
        return k.value, rows.value, bool(dense.value)

    def residual_cvec(self, b, y, r):
        check(lib.pmg_grid_residual_cvec(self._h, _ptr(b), _ptr(y), _ptr(r), _stream()))

    def destroy(self):
        if self._h:
            check(lib.pmg_grid_destroy(C.byref(self._h)))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class CholSampler:
    """Exact coarse sampler (reference PCCHOLSAMPLER dense path, src/pc_chols.c:174-291)."""

    def __init__(self, rowptr, colidx, vals, B=None, S=None, idx_width=32):
        """B (n x k), S (k): factor the MATLRC operator A + B diag(S) B^T instead (src/pc_chols.c:119-153)."""
        it = np.int64 if idx_width == 64 else np.int32
        rp, ci, v = np.ascontiguousarray(rowptr, it), np.ascontiguousarray(colidx, it), np.ascontiguousarray(vals, np.float64)
        self.n = len(rp) - 1
        self._h = C.c_void_p()
        if idx_width != 32:
            k = 0 if B is None else np.asarray(B).shape[1]
            Bf = None if B is None else np.asfortranarray(B, np.float64)
            Sf = None if S is None else np.ascontiguousarray(S, np.float64)
            check(lib.pmg_chol_create_csr_idx(self.n, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, idx_width, k, None if Bf is None else Bf.ctypes.data, None if Sf is None else Sf.ctypes.data, C.byref(self._h)))
        elif B is None:
            check(lib.pmg_chol_create_csr(self.n, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, C.byref(self._h)))
        else:
            B = np.asfortranarray(B, np.float64)
            S = np.ascontiguousarray(S, np.float64)
            assert B.shape == (self.n, len(S))
            check(lib.pmg_chol_create_csr_lowrank(self.n, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, B.shape[1], B.ctypes.data, S.ctypes.data, C.byref(self._h)))

    def factor(self) -> np.ndarray:
        out = np.zeros(self.n * self.n)
        check(lib.pmg_chol_get_factor(self._h, out.ctypes.data))
        return out.reshape((self.n, self.n), order="F")

    def sample(self, b, y, seed: int = 0, counter: int = 0, noisy: bool = True):
        check(lib.pmg_chol_sample(self._h, _ptr(b), _ptr(y), int(noisy), seed, counter, _stream()))

    def destroy(self):
        if self._h:
            check(lib.pmg_chol_destroy(C.byref(self._h)))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def _blocks(blocks):
    """(nblocks, blockptr, blockrows) int32 arrays of a sequence of row lists, or of a (blockptr, blockrows) pair as is"""
    if isinstance(blocks, tuple) and len(blocks) == 2 and isinstance(blocks[0], np.ndarray):
        bp, br = blocks
    else:
        bp = np.concatenate([[0], np.cumsum([len(p) for p in blocks])])
        br = np.concatenate([np.asarray(p, np.int64) for p in blocks]) if len(blocks) else np.zeros(0)
    bp, br = np.ascontiguousarray(bp, np.int32), np.ascontiguousarray(br, np.int32)
    return len(bp) - 1, bp, br


class MGMC:
    """Multigrid Monte Carlo on a DMDA hierarchy (reference PCGAMGMC, src/pc_gamgmc.c, with -pc_gamgmc_mg_type mg)."""

    def __init__(self, nx, ny, nz, kappa, levels, keep_host=False):
        self.nx, self.ny, self.nz, self.n = nx, ny, nz, nx * ny * nz
        self._h = C.c_void_p()
        check(lib.pmg_mgmc_create_dmda(nx, ny, nz, kappa, levels, C.byref(self._h)))
        check(lib.pmg_mgmc_set_keep_host(self._h, int(keep_host)))
        self.levels = levels

    @classmethod
    def from_hierarchy(cls, operators, interpolations, idx_width=32):
        """operators[l] = (rowptr, colidx, vals) of level l (0 = coarsest); interpolations[l] (l >= 1) = CSR triple of
        the prolongation from level l-1 to level l (reference src/pc_gamgmc.c:165-176: what PCMG holds).  idx_width 64:
        the index arrays cross the boundary as 64-bit PetscInt and need not outlive the calls."""
        self = cls.__new__(cls)
        levels = len(operators)
        self._h = C.c_void_p()
        self.levels = levels
        self._keep = []
        it = np.int64 if idx_width == 64 else np.int32
        check(lib.pmg_mgmc_create_hierarchy(levels, C.byref(self._h)))
        for l, (rp, ci, v) in enumerate(operators):
            rp, ci, v = np.ascontiguousarray(rp, it), np.ascontiguousarray(ci, it), np.ascontiguousarray(v, np.float64)
            self._keep.append((rp, ci, v) if idx_width == 32 else (v,))
            if idx_width == 32:
                check(lib.pmg_mgmc_set_level_operator(self._h, l, len(rp) - 1, rp.ctypes.data, ci.ctypes.data, v.ctypes.data))
            else:
                check(lib.pmg_mgmc_set_level_operator_idx(self._h, l, len(rp) - 1, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, idx_width))
        for l in range(1, levels):
            rp, ci, v = interpolations[l]
            rp, ci, v = np.ascontiguousarray(rp, it), np.ascontiguousarray(ci, it), np.ascontiguousarray(v, np.float64)
            self._keep.append((rp, ci, v) if idx_width == 32 else (v,))
            nc = len(operators[l - 1][0]) - 1
            if idx_width == 32:
                check(lib.pmg_mgmc_set_level_interpolation(self._h, l, len(rp) - 1, nc, rp.ctypes.data, ci.ctypes.data, v.ctypes.data))
            else:
                check(lib.pmg_mgmc_set_level_interpolation_idx(self._h, l, len(rp) - 1, nc, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, idx_width))
        self.n = len(operators[-1][0]) - 1
        return self

    def set_smoother(self, scaled: bool, omega: float = 1.0, sweep_type: int = capi.SOR_FORWARD_SWEEP, its: int = 1):
        check(lib.pmg_mgmc_set_smoother(self._h, int(scaled), omega, sweep_type, its))

    def set_correction_form(self, literal: bool):
        check(lib.pmg_mgmc_set_correction_form(self._h, int(literal)))

    def set_fused_transfers(self, on: bool):
        """False: residual and restriction as two kernels, a low-rank term subtracted before the restriction (the
        reference's operation order); True (default): the fused kernel and the restricted low-rank term."""
        check(lib.pmg_mgmc_set_fused_transfers(self._h, int(on)))

    def set_coloring(self, rule: int):
        """colouring rule of the AIJ levels (capi.COLORING_GREEDY, the default, or capi.COLORING_ITERATED); before setup"""
        check(lib.pmg_mgmc_set_coloring(self._h, int(rule)))

    def set_lowrank(self, B, S):
        """MATLRC fine operator A + B diag(S) B^T, propagated to every level (reference src/pc_gamgmc.c:157-196)."""
        B = np.asfortranarray(B, np.float64)
        S = np.ascontiguousarray(S, np.float64)
        assert B.ndim == 2 and B.shape[1] == len(S)
        check(lib.pmg_mgmc_set_lowrank(self._h, B.shape[1], B.ctypes.data, S.ctypes.data))

    def set_level_blocks(self, level: int, blocks, block_colors=None):
        """smooth `level` of a from_hierarchy handle with block Gibbs sweeps over `blocks` (as BlockGibbs); before setup"""
        nb, bp, br = _blocks(blocks)
        bc = None if block_colors is None else np.ascontiguousarray(block_colors, np.int32)
        nc = 0 if bc is None or not len(bc) else int(bc.max()) + 1
        check(lib.pmg_mgmc_set_level_blocks(self._h, level, nb, bp.ctypes.data, br.ctypes.data, nc, None if bc is None else bc.ctypes.data))

    def set_coarse(self, kind: str = "cholsampler", its: int = 1):
        check(lib.pmg_mgmc_set_coarse(self._h, {"cholsampler": 0, "gibbs": 1}[kind], its))

    def setup(self):
        check(lib.pmg_mgmc_setup(self._h))
        return self

    def level_dims(self, level: int):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib.pmg_mgmc_get_level_dims(self._h, level, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def level_matrix(self, level: int, which: str):
        w = {"A": 0, "P": 1}[which]
        nr, nnz = C.c_int32(), C.c_int32()
        check(lib.pmg_mgmc_get_level_matrix(self._h, level, w, C.byref(nr), C.byref(nnz), None, None, None))
        rp, ci, v = np.zeros(nr.value + 1, np.int32), np.zeros(nnz.value, np.int32), np.zeros(nnz.value)
        check(lib.pmg_mgmc_get_level_matrix(self._h, level, w, C.byref(nr), C.byref(nnz), rp.ctypes.data, ci.ctypes.data, v.ctypes.data))
        return rp, ci, v

    # --- one kernel of the V-cycle on caller vectors in the level's own layout (diagnostics for full-size parity tests) ---
    def level_layout(self, level: int):
        """(kind, ld, off): kind 0 = grid cvec, 1 = class stencil, 2 = sliced-ELL, 3 = dense coarsest; natural index q of
        kinds 1 and 3 sits at off + q"""
        k, ld, off = C.c_int32(), C.c_int64(), C.c_int64()
        check(lib.pmg_mgmc_get_level_layout(self._h, level, C.byref(k), C.byref(ld), C.byref(off)))
        return k.value, ld.value, off.value

    def level_stencil(self, level: int):
        coef, sq = np.zeros((27, 27)), np.zeros(27)
        check(lib.pmg_mgmc_get_level_stencil(self._h, level, coef.ctypes.data, sq.ctypes.data))
        return coef, sq

    def level_sweep(self, level: int, b, x, backward: bool = False, noisy: bool = False, seed: int = 0, counter: int = 0):
        check(lib.pmg_mgmc_level_sweep(self._h, level, int(backward), int(noisy), seed, counter, _ptr(b), _ptr(x), _stream()))

    def level_residual(self, level: int, b, x, r):
        check(lib.pmg_mgmc_level_residual(self._h, level, _ptr(b), _ptr(x), _ptr(r), _stream()))

    def level_restrict(self, level: int, r_fine, b_coarse):
        check(lib.pmg_mgmc_level_restrict(self._h, level, _ptr(r_fine), _ptr(b_coarse), _stream()))

    def level_residual_restrict(self, level: int, b, x, b_coarse):
        check(lib.pmg_mgmc_level_residual_restrict(self._h, level, _ptr(b), _ptr(x), _ptr(b_coarse), _stream()))

    def level_prolong_add(self, level: int, e_coarse, x_fine):
        check(lib.pmg_mgmc_level_prolong_add(self._h, level, _ptr(e_coarse), _ptr(x_fine), _stream()))

    def algorithmic_bytes(self):
        """(total, per_level): algorithmic bytes of one sample as the cycle is built (pmg_mgmc_get_algorithmic_bytes)"""
        tot = C.c_double()
        per = np.zeros(self.levels)
        check(lib.pmg_mgmc_get_algorithmic_bytes(self._h, C.byref(tot), per.ctypes.data))
        return tot.value, per

    def level_lowrank_factors(self, level: int):
        """(rows, B, Bb_fwd, Bb_bwd): layout positions of the support rows and the ns x k blocks the kernels use"""
        k, ns = C.c_int32(), C.c_int64()
        check(lib.pmg_mgmc_level_lowrank_factors(self._h, level, C.byref(k), C.byref(ns), None, None, None, None))
        rows = np.zeros(ns.value, np.int64)
        B, Bf, Bb = (np.zeros((ns.value, k.value), order="F") for _ in range(3))
        check(lib.pmg_mgmc_level_lowrank_factors(self._h, level, C.byref(k), C.byref(ns), rows.ctypes.data, B.ctypes.data, Bf.ctypes.data, Bb.ctypes.data))
        return rows, B, Bf, Bb

    def level_lowrank_sizes(self, level: int):
        """(k, rows, dense): rank of the level's update and the rows its passes run over, on every kind of level"""
        k, rows, dense = C.c_int32(), C.c_int64(), C.c_int()
        check(lib.pmg_mgmc_level_lowrank_sizes(self._h, level, C.byref(k), C.byref(rows), C.byref(dense)))
        return k.value, rows.value, bool(dense.value)

    def level_lowrank_post(self, level: int, y, backward: bool = False):
        check(lib.pmg_mgmc_level_lowrank_post(self._h, level, int(backward), _ptr(y), _stream()))

    def level_lowrank_residual_sub(self, level: int, x, out, restricted: bool = False):
        check(lib.pmg_mgmc_level_lowrank_residual_sub(self._h, level, int(restricted), _ptr(x), _ptr(out), _stream()))

    def sample(self, b, y, its: int, seed: int, counter0: int = 0, guesszero: bool = False, callback=None, stats=None, rb=None) -> int:
        """stats: a ChainStats of one chain, updated after every sample by the library's own callback (no Python in the loop);
        rb: an RBStats of one chain, the same way; both together are updated by one Python-level callback"""
        out = C.c_uint64()
        if stats is not None or rb is not None:
            if callback is not None:
                raise ValueError("stats= / rb= and callback= exclude each other")
            if stats is not None and rb is not None:
                callback = _update_all(self.n, 1, stats, rb)
            else:
                cb, ctx = stats._as_callback(self.n, 1, lib.pmg_chainstats_sample_callback) if rb is None else rb._as_callback(self.n, 1, lib.pmg_rbstats_sample_callback)
                check(lib.pmg_mgmc_sample(self._h, _ptr(b), _ptr(y), its, int(guesszero), seed, counter0, C.byref(out), cb, ctx, _stream()))
                return out.value
        if callback is None:
            cb = None
        else:
            import torch

            def _cb(it, ptr, n, _ctx):
                try:
                    callback(it, y)  # y is the tensor the library writes the sample into
                    return 0
                except Exception:  # pragma: no cover
                    import traceback

                    traceback.print_exc()
                    return 77

            cb = capi.SAMPLE_CALLBACK(_cb)
        check(lib.pmg_mgmc_sample(self._h, _ptr(b), _ptr(y), its, int(guesszero), seed, counter0, C.byref(out), cb, None, _stream()))
        return out.value

    def sample_chains(self, b, Y, its: int, seeds, counter0: int = 0, guesszero: bool = False, callback=None, stats=None, cov=None, rb=None) -> int:
        """`its` samples of C chains on a hierarchy from from_hierarchy: Y is a contiguous (n, C) float64 tensor, b one vector
        (n,) shared by all chains or one per chain (n, C); column c equals sample(b or b[:, c], Y[:, c], its, seeds[c], ...) bit
        for bit.  callback(it, Y) after every sample; a raised exception aborts the loop.  stats: a ChainStats(n, C) updated
        after every sample by the library's own callback instead (no Python in the loop; excludes callback).  cov: a
        ChainCov(n, C) that records the covariance error of every sample the same way; rb: an RBStats(A, C) updated the same way;
        two or three of stats=, cov= and rb= together are updated by one Python-level callback.  A hierarchy with set_lowrank
        samples the posterior A + B diag(S) B^T the same way (after setup)."""
        p, nc = _chains(Y, self.n)
        s = _seeds(seeds, nc)
        out = C.c_uint64()
        cb, ctx = None, None
        consumers = [x for x in (stats, cov, rb) if x is not None]
        if consumers and callback is not None:
            raise ValueError("stats= / cov= / rb= and callback= exclude each other")
        if len(consumers) > 1:
            callback = _update_all(self.n, nc, *consumers)
        elif stats is not None:
            cb, ctx = stats._as_callback(self.n, nc, lib.pmg_chainstats_callback)
        elif cov is not None:
            cb, ctx = cov._as_callback(self.n, nc)
        elif rb is not None:
            cb, ctx = rb._as_callback(self.n, nc, lib.pmg_rbstats_callback)
        if callback is not None:

            def _cb(it, ptr, n, nchains, _ctx):
                try:
                    callback(it, Y)
                    return 0
                except Exception:  # pragma: no cover
                    import traceback

                    traceback.print_exc()
                    return 77

            cb = capi.CHAINS_CALLBACK(_cb)
        fn = lib.pmg_mgmc_sample_chains_rhs if _per_chain_rhs(b, self.n, nc) else lib.pmg_mgmc_sample_chains
        check(fn(self._h, nc, s.ctypes.data, _ptr(b), p, its, int(guesszero), counter0, C.byref(out), cb, ctx, _stream()))
        return out.value

    def algorithmic_bytes_chains(self, nchains: int):
        """(total, per_level): algorithmic bytes of one V-cycle advancing `nchains` chains (pmg_mgmc_get_algorithmic_bytes_chains)"""
        tot = C.c_double()
        per = np.zeros(self.levels)
        check(lib.pmg_mgmc_get_algorithmic_bytes_chains(self._h, nchains, C.byref(tot), per.ctypes.data))
        return tot.value, per

    def destroy(self):
        if self._h:
            check(lib.pmg_mgmc_destroy(C.byref(self._h)))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class WoodburySampler:
    """PCWOODBURY (reference src/woodbury.c): posterior sampler for A + B diag(S) B^T from ANY sampler of A plus a solver --
    on one device or on rows distributed over ranks (z-slabs, row blocks): B_rows = this rank's rows of B (n x k), vectors in
    natural order over those rows; `dist_handle` = the C handle of a transport of the ranks (ctypes void pointer) or None.
      solve(b, x)            x <- (approximately) A^-1 b from the zero guess x holds (device tensors), collective
      sample(w, y, counter)  one sample of the A-sampler on right-hand side w, y updated in place, collective
      sample_chains(W, Y, counter)  (optional, one device) the same on C chains: column c of Y advanced on W[:, c] (run_chains)"""

    def __init__(self, B_rows, S, solve, sample, dist_handle=None, sample_chains=None):
        import torch

        B = np.asfortranarray(B_rows, np.float64)
        S = np.ascontiguousarray(S, np.float64)
        self.n, self.k = B.shape
        assert len(S) == self.k
        self._h = C.c_void_p()
        self._sample = sample
        self._sample_chains = sample_chains
        self._W = None
        check(lib.pmg_woodbury_create(self.n, self.k, B.ctypes.data, max(self.n, 1), S.ctypes.data, dist_handle, C.byref(self._h)))
        for c in range(self.k):  # C = solver(B) column by column from a zero guess (src/woodbury.c:35-50)
            b = torch.as_tensor(np.ascontiguousarray(B[:, c]), device="cuda")
            x = torch.zeros(self.n, dtype=torch.float64, device="cuda")
            solve(b, x)
            check(lib.pmg_woodbury_set_c_column(self._h, c, _ptr(x), _stream()))
        torch.cuda.synchronize()
        check(lib.pmg_woodbury_finish(self._h))
        self._w = torch.zeros(self.n, dtype=torch.float64, device="cuda")

    def correction(self):
        G = np.zeros((self.n, self.k), order="F")
        check(lib.pmg_woodbury_get_correction(self._h, G.ctypes.data))
        return G

    def run(self, b, y, its: int, seed: int, counter0: int = 0, callback=None) -> int:
        """PCApplyRichardson_Woodbury (src/woodbury.c:263-289); sample `it` uses noise counter counter0 + it for the k-vector
        and hands the same counter to the A-sampler"""
        for it in range(its):
            check(lib.pmg_woodbury_noisy_rhs(self._h, _ptr(b), _ptr(self._w), seed ^ 0x5851F42D4C957F2D, counter0 + it, _stream()))
            self._sample(self._w, y, counter0 + it)
            check(lib.pmg_woodbury_correct(self._h, _ptr(y), _stream()))
            if callback is not None:
                callback(it, y)
        return counter0 + its

    def run_chains(self, b, Y, its: int, seeds, counter0: int = 0, callback=None, sample_chains=None, stats=None, cov=None, rb=None) -> int:
        """run() on C chains of one device: Y is a contiguous (n, C) float64 tensor, b one vector (n,) shared by the chains;
        column c equals run(b, Y[:, c], its, seeds[c], counter0) bit for bit when sample_chains(W, Y, counter) advances every
        column c of Y as sample(W[:, c], Y[:, c], counter) does -- e.g. MGMC.sample_chains with per-chain right-hand sides.
        callback(it, Y) after every sample, or stats.update(Y) for a ChainStats(n, C), cov.update(Y) for a ChainCov(n, C) and
        rb.update(Y) for an RBStats built on (A, B, S) with this b (not both kinds)."""
        import torch

        if (stats is not None or cov is not None or rb is not None) and callback is not None:
            raise ValueError("stats= / cov= / rb= and callback= exclude each other")
        p, nc = _chains(Y, self.n)
        if cov is not None:
            cov._check_sizes(self.n, nc)
        if rb is not None:
            rb._check_sizes(self.n, nc)
        sample_chains = sample_chains or self._sample_chains
        assert sample_chains is not None, "run_chains needs sample_chains(W, Y, counter)"
        keys = _seeds([int(v) ^ 0x5851F42D4C957F2D for v in _seeds(seeds, nc)], nc)
        if getattr(self, "_W", None) is None or tuple(self._W.shape) != (self.n, nc):
            self._W = torch.empty((self.n, nc), dtype=torch.float64, device="cuda")
        for it in range(its):
            check(lib.pmg_woodbury_noisy_rhs_chains(self._h, nc, keys.ctypes.data, counter0 + it, _ptr(b), _ptr(self._W), _stream()))
            sample_chains(self._W, Y, counter0 + it)
            check(lib.pmg_woodbury_correct_chains(self._h, nc, p, _stream()))
            if stats is not None:
                stats.update(Y)
            if cov is not None:
                cov.update(Y)
            if rb is not None:
                rb.update(Y)
            if callback is not None:
                callback(it, Y)
        return counter0 + its

    def destroy(self):
        if self._h:
            check(lib.pmg_woodbury_destroy(C.byref(self._h)))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class ChainStats:
    """pmg_chainstats: running mean and variance of every row over all steps x chains samples, the quantities of interest
    w_q . Y[:, c] of every chain per step and R-hat on them, kept on the device (replaces the host loops of the reference's
    examples/ex7.c:40-93, src/ms.c:221-251 and examples/benchmark/main.cc:151-175).
      qois: a list with one entry per QOI -- None for all ones (VecSum) or n weights (VecDot); at most 4 entries."""

    def __init__(self, n: int, nchains: int = 1, qois=(), max_steps: int = 1000):
        qois = list(qois)
        self.n, self.nchains, self.nqoi, self.max_steps = int(n), int(nchains), len(qois), int(max_steps)
        self._h = C.c_void_p()
        check(lib.pmg_chainstats_create(self.n, self.nchains, self.nqoi, self.max_steps, C.byref(self._h)))
        for q, w in enumerate(qois):
            self.set_qoi(q, w)

    def set_qoi(self, q: int, w=None):
        if w is None:
            check(lib.pmg_chainstats_set_qoi(self._h, q, None))
            return
        w = np.ascontiguousarray(w.detach().cpu().numpy() if hasattr(w, "detach") else w, np.float64)
        assert w.shape == (self.n,), f"need {self.n} weights"
        check(lib.pmg_chainstats_set_qoi(self._h, q, w.ctypes.data))

    def update(self, Y):
        """one step: Y is a contiguous (n, C) float64 CUDA tensor (or (n,) for one chain), on the current stream"""
        assert Y.numel() == self.n * self.nchains and (Y.dim() == 1 or tuple(Y.shape) == (self.n, self.nchains)), f"need an ({self.n}, {self.nchains}) tensor"
        check(lib.pmg_chainstats_update(self._h, _ptr(Y), _stream()))

    def _as_callback(self, n: int, nchains: int, fn):
        """(function pointer, context) for a sampler's callback argument; the callback launches on the current stream"""
        assert (n, nchains) == (self.n, self.nchains), f"ChainStats of {self.n} x {self.nchains} on samples of {n} x {nchains}"
        check(lib.pmg_chainstats_set_stream(self._h, _stream()))
        return C.cast(fn, C.c_void_p), self._h

    def reset(self):
        check(lib.pmg_chainstats_reset(self._h))

    def count(self):
        """(steps, samples = steps * chains)"""
        st, sm = C.c_int32(), C.c_int64()
        check(lib.pmg_chainstats_get_count(self._h, C.byref(st), C.byref(sm)))
        return st.value, sm.value

    def fields(self):
        """(mean, var): device tensors of n entries, the unbiased variance over all samples seen"""
        import torch

        mean = torch.empty(self.n, dtype=torch.float64, device="cuda")
        var = torch.empty(self.n, dtype=torch.float64, device="cuda")
        check(lib.pmg_chainstats_get_fields(self._h, _ptr(mean), _ptr(var), _stream()))
        return mean, var

    def trace(self, q: int = 0, first: int = 0, count=None) -> np.ndarray:
        """QOI q of the steps [first, first + count) as a host array (count, C); count = None: all recorded steps from first"""
        if count is None:
            count = max(self.count()[0] - first, 0)
        out = np.empty((max(count, 0), self.nchains))
        check(lib.pmg_chainstats_get_trace(self._h, q, first, count, out.ctypes.data))
        return out

    def rhat(self, q: int = 0, first: int = 0, count=None) -> float:
        """Gelman-Rubin R-hat (examples/ex7.c:61-93) of QOI q over the steps [first, first + count)"""
        if count is None:
            count = max(self.count()[0] - first, 0)
        gr = C.c_double()
        check(lib.pmg_chainstats_rhat(self._h, q, first, count, C.byref(gr)))
        return gr.value

    def iact(self, q: int = 0, first: int = 0, count=None):
        """pmg_iact of every chain's trace of QOI q: a list of (tau, valid), one per chain"""
        t = self.trace(q, first, count)
        return [iact(t[:, c]) for c in range(self.nchains)]

    def iact_device(self, q: int = 0, first: int = 0, count=None, max_lag: int = 0, nacf: int = 0):
        """pmg_chainstats_iact: the IACT of every chain's trace of QOI q over the steps [first, first + count), computed where
        the trace lies.  Returns (tau, window, valid), numpy arrays of one entry per chain, and with nacf > 0 also the
        autocorrelation as an (nacf, C) device tensor.  max_lag = 0: no limit; see iact_chains."""
        if count is None:
            count = max(self.count()[0] - first, 0)
        return _iact_call(self.nchains, nacf, lambda tau, win, val, acf: lib.pmg_chainstats_iact(self._h, q, first, count, max_lag, tau, win, val, nacf, acf, _stream()))

    def destroy(self):
        if self._h:
            check(lib.pmg_chainstats_destroy(C.byref(self._h)))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class ChainCov:
    """pmg_chaincov: the covariance error of every step's chains against a dense reference, kept on the device --
    err[step] = ||C_step - Sigma||_F / ||Sigma||_F with C_step the unbiased covariance over the chains (replaces
    EstimateCovarianceMatErrors, reference src/stats.c:94-117, on the host copies of examples/ex6.c:168-193).  Build with
    from_chol / from_csr (Sigma = the inverse of the factored matrix, formed on the device) or from_dense (any symmetric Sigma)."""

    def __init__(self, handle, n: int, nchains: int, max_steps: int):
        self._h, self.n, self.nchains, self.max_steps = handle, int(n), int(nchains), int(max_steps)

    @classmethod
    def from_chol(cls, chol, nchains: int, max_steps: int = 1000):
        """Sigma = L^-T L^-1 of a CholSampler (prior, or posterior when it was built with B, S); chol may be destroyed afterwards"""
        h = C.c_void_p()
        check(lib.pmg_chaincov_create_chol(chol._h, nchains, max_steps, C.byref(h)))
        return cls(h, chol.n, nchains, max_steps)

    @classmethod
    def from_csr(cls, rowptr, colidx, vals, nchains: int, max_steps: int = 1000, lowrank=None):
        """Sigma = A^-1, or (A + B diag(S) B^T)^-1 with lowrank = (B, S)"""
        B, S = lowrank if lowrank is not None else (None, None)
        chol = CholSampler(rowptr, colidx, vals, B, S)
        try:
            return cls.from_chol(chol, nchains, max_steps)
        finally:
            chol.destroy()

    @classmethod
    def from_dense(cls, Sigma, nchains: int, max_steps: int = 1000):
        """any symmetric (n, n) reference on the host; uploaded by the first update"""
        Sg = np.ascontiguousarray(Sigma, np.float64)
        assert Sg.ndim == 2 and Sg.shape[0] == Sg.shape[1], "need a square matrix"
        h = C.c_void_p()
        check(lib.pmg_chaincov_create_dense(Sg.shape[0], Sg.ctypes.data, nchains, max_steps, C.byref(h)))
        return cls(h, Sg.shape[0], nchains, max_steps)

    def _check_sizes(self, n: int, nchains: int):
        assert (n, nchains) == (self.n, self.nchains), f"ChainCov of {self.n} x {self.nchains} on samples of {n} x {nchains}"

    def update(self, Y):
        """one step: Y is a contiguous (n, C) float64 CUDA tensor, on the current stream"""
        assert tuple(Y.shape) == (self.n, self.nchains), f"need an ({self.n}, {self.nchains}) tensor"
        check(lib.pmg_chaincov_update(self._h, _ptr(Y), _stream()))

    def _as_callback(self, n: int, nchains: int):
        """(function pointer, context) for a sampler's chains callback; the callback launches on the current stream"""
        self._check_sizes(n, nchains)
        check(lib.pmg_chaincov_set_stream(self._h, _stream()))
        return C.cast(lib.pmg_chaincov_callback, C.c_void_p), self._h

    def reset(self):
        check(lib.pmg_chaincov_reset(self._h))

    def count(self) -> int:
        st = C.c_int32()
        check(lib.pmg_chaincov_get_count(self._h, C.byref(st)))
        return st.value

    def errors(self, first: int = 0, count=None) -> np.ndarray:
        """the errors of the steps [first, first + count) as a host array; count = None: all recorded steps from first"""
        if count is None:
            count = max(self.count() - first, 0)
        out = np.empty(max(count, 0))
        check(lib.pmg_chaincov_get_errors(self._h, first, count, out.ctypes.data))
        return out

    def reference(self) -> np.ndarray:
        """Sigma as a host (n, n) array"""
        out = np.empty((self.n, self.n))
        check(lib.pmg_chaincov_get_reference(self._h, out.ctypes.data))
        return out

    def covariance(self, Y):
        """the unbiased covariance over the chains of one step as an (n, n) device tensor (both triangles); records nothing"""
        import torch

        assert tuple(Y.shape) == (self.n, self.nchains), f"need an ({self.n}, {self.nchains}) tensor"
        out = torch.empty((self.n, self.n), dtype=torch.float64, device="cuda")
        check(lib.pmg_chaincov_covariance(self._h, _ptr(Y), _ptr(out), _stream()))
        return out

    def destroy(self):
        if self._h:
            check(lib.pmg_chaincov_destroy(C.byref(self._h)))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def _update_all(n: int, nchains: int, *consumers):
    """a Python-level callback that feeds several of ChainStats, ChainCov and RBStats of the sampler's sizes, in the order given"""
    for x in consumers:
        assert (n, nchains) == (x.n, x.nchains), f"{type(x).__name__} of {x.n} x {x.nchains} on samples of {n} x {nchains}"

    def update_all(it, Y):
        for x in consumers:
            x.update(Y)

    return update_all


def gelman_rubin(vals) -> float:
    """GelmanRubin (reference examples/ex7.c:61-93): vals is (chains, n), host arithmetic in the reference's order"""
    v = np.ascontiguousarray(vals, np.float64)
    assert v.ndim == 2
    gr = C.c_double()
    check(lib.pmg_gelman_rubin(v.shape[0], v.shape[1], v.ctypes.data, C.byref(gr)))
    return gr.value


def vec_set_random_standard_normal(x, seed: int, counter: int = 0):
    """VecSetRandomStandardNormal (reference src/parmgmc.c:70-116) on the counter-based source."""
    check(lib.pmg_vec_set_random_standard_normal(x.numel(), _ptr(x), seed, counter, _stream()))
    return x


def autocorrelation(x):
    """Autocorrelation (reference src/iact.c:17-47) of a scalar series; host arrays."""
    x = np.ascontiguousarray(x, np.float64)
    acf = np.empty_like(x)
    check(lib.pmg_autocorrelation(len(x), x.ctypes.data, acf.ctypes.data))
    return acf


def iact(x):
    """IACT (reference src/iact.c:73-92): returns (tau, valid)."""
    x = np.ascontiguousarray(x, np.float64)
    tau, valid = C.c_double(), C.c_int()
    check(lib.pmg_iact(len(x), x.ctypes.data, C.byref(tau), None, C.byref(valid)))
    return tau.value, bool(valid.value)


IACT_LAG_BLOCK = 256  # PMG_IACT_LAG_BLOCK: lags per block of the device scan


def _iact_call(nseries: int, nacf: int, call):
    """the host outputs and the optional acf tensor of the two device IACT entry points around one library call"""
    tau, window, valid = np.empty(nseries), np.empty(nseries, np.int32), np.empty(nseries, np.int32)
    acf = None
    if nacf > 0:
        import torch

        acf = torch.empty((nacf, nseries), dtype=torch.float64, device="cuda")
    check(call(tau.ctypes.data, window.ctypes.data, valid.ctypes.data, _ptr(acf) if acf is not None else None))
    out = (tau, window, valid.astype(bool))
    return out + (acf,) if acf is not None else out


def iact_chains(X, max_lag: int = 0, nacf: int = 0):
    """pmg_iact_chains: IACT (reference src/iact.c:73-92) of every column of an (n, S) float64 CUDA tensor -- rows are steps,
    columns are series; a column slice of a wider contiguous tensor is taken where it lies.  Returns (tau, window, valid), numpy
    arrays of S entries, and with nacf > 0 also the autocorrelation of the first nacf lags as an (nacf, S) device tensor.
    max_lag = 0: no limit, the reference's rule; max_lag > 0: a series without a window up to max_lag reports window = -1,
    tau = T_max_lag, valid = False.  Runs on the current stream and synchronises it."""
    import torch

    assert isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float64 and X.dim() == 2, "need an (n, S) float64 CUDA tensor"
    n, S = (int(v) for v in X.shape)
    assert S == 1 or X.stride(1) == 1, "the series of a step must be adjacent in memory"
    ld = int(X.stride(0)) if n > 1 else S
    return _iact_call(S, nacf, lambda tau, win, val, acf: lib.pmg_iact_chains(n, S, C.c_void_p(X.data_ptr()), ld, max_lag, tau, win, val, nacf, acf, _stream()))


def estimate_covariance_errors(rowptr, colidx, vals, samples, chains: int):
    """EstimateCovarianceMatErrors (reference src/stats.c:94-117); samples: (samples_per_chain * chains, n) host rows
    ordered sample-major."""
    rp, ci, v = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colidx, np.int32), np.ascontiguousarray(vals, np.float64)
    S = np.ascontiguousarray(samples, np.float64)
    n = len(rp) - 1
    assert S.ndim == 2 and S.shape[1] == n and S.shape[0] % chains == 0
    spc = S.shape[0] // chains
    errs = np.empty(spc)
    check(lib.pmg_estimate_covariance_errors(n, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, chains, spc, S.ctypes.data, errs.ctypes.data))
    return errs


def make_observation_mats(nx, ny, nz, coords, radii, obsvals, sigma2, kz0=0, nz_owned=None):
    """MakeObservationMats (reference src/obs.c:135-180) on the unit-cube DMDA: returns (B, S, f) as host arrays, rows =
    the planes [kz0, kz0 + nz_owned) in natural order."""
    nz_owned = nz if nz_owned is None else nz_owned
    coords = np.ascontiguousarray(coords, np.float64).ravel()
    radii = np.ascontiguousarray(radii, np.float64)
    vals = np.ascontiguousarray(obsvals, np.float64)
    k, n = len(radii), nx * ny * nz_owned
    B = np.zeros((n, k), order="F")
    S, f = np.zeros(k), np.zeros(n)
    check(lib.pmg_make_observation_mats_dmda(nx, ny, nz, kz0, nz_owned, k, sigma2, coords.ctypes.data, radii.ctypes.data, vals.ctypes.data, B.ctypes.data, S.ctypes.data, f.ctypes.data))
    return B, S, f


from .rbstats import RBStats  # noqa: E402,F401  (its own module; needs _ptr and _stream above)
