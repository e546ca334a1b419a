"""Blocks, a plain numpy reference and a kernel-order walk-through for the coloured block Gibbs sampler (pmg_blockgibbs,
kernels_blockgibbs.hip).  Helpers only.

One patch update (reference examples/ex13.py:11-22: PCASM multiplicative around -sub_pc_type cholsampler,
src/pc_chols.c:174-194,220-260) is  y_P <- A_PP^-1 (b_P - A_{P,rest} y_rest) + L_P^-T xi_P,  A_PP = L_P L_P^T.

  ref_sweep      the reference: blocks in (colour, index) order, np.linalg.cholesky and two triangular solves per block.  With
                 bound=True it also returns a rigorous running bound on what a backward-stable implementation may differ by
                 (see its docstring); the GPU tests hold the walk-through to it.
  walk_sweep     the kernel's order of operations, restated with the library's own W = L^-1 (pmg_blockgibbs_get_block_factor):
                 r_i = b[p_i] - sum a_k y[col_k] over the stored entries outside the block in storage order, M = W^T W summed
                 over k ascending, y_i = sum_j M_ij r_j (+ sum_j W_ji xi_j), j ascending from zero, products and sums rounded
                 separately.  The device must equal it bit for bit.
  noise_bound    how far a chain drawn on the device may be from the same chain fed the oracle's normals.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import oracle as O
from chol_edge_refs import U, fwd_bound, gamma

FWD, BWD, SYM = O.SOR_FORWARD, O.SOR_BACKWARD, O.SOR_SYMMETRIC


# ---- operators -----------------------------------------------------------------------------------------------------------
def squared(A: O.CSR) -> O.CSR:
    return O.CSR.from_scipy(A.scipy() @ A.scipy())


def banded(n=300, half_bandwidth=70, seed=11) -> O.CSR:
    """symmetric, every entry within the band stored, strictly diagonally dominant with a positive diagonal: SPD"""
    rng = np.random.default_rng(seed)
    M = np.zeros((n, n))
    for d in range(1, half_bandwidth + 1):
        v = -rng.uniform(0.1, 1.0, n - d)
        M += np.diag(v, d) + np.diag(v, -d)
    M += np.diag(np.abs(M).sum(axis=1) + 1.0)
    return O.CSR.from_scipy(sp.csr_matrix(M))


def two_components(n1=9, n2=40, seed=12) -> O.CSR:
    """a dense SPD clique of n1 rows next to a tridiagonal chain of n2 rows, not coupled to each other"""
    rng = np.random.default_rng(seed)
    C = -rng.uniform(0.1, 1.0, (n1, n1))
    C = np.triu(C, 1) + np.triu(C, 1).T
    C += np.diag(np.abs(C).sum(axis=1) + 1.0)
    v = -rng.uniform(0.1, 1.0, n2 - 1)
    T = np.diag(v, 1) + np.diag(v, -1)
    T += np.diag(np.abs(T).sum(axis=1) + 1.0)
    return O.CSR.from_scipy(sp.block_diag([sp.csr_matrix(C), sp.csr_matrix(T)]))


# ---- block builders ------------------------------------------------------------------------------------------------------
def star_blocks(pattern: O.CSR):
    """vertex stars: block v = the columns row v of `pattern` stores, in storage order (overlapping)"""
    return [pattern.colidx[pattern.rowptr[v]:pattern.rowptr[v + 1]].astype(np.int64) for v in range(pattern.n)]


def cell_blocks(nx, ny, nz=1):
    """2 x 2 (x 2) cells starting at even indices, clipped at the far faces: 1 to 4 (8) rows, disjoint"""
    out = []
    for k0 in range(0, nz, 2):
        for j0 in range(0, ny, 2):
            for i0 in range(0, nx, 2):
                out.append(np.array([i + nx * (j + ny * k) for k in range(k0, min(k0 + 2, nz)) for j in range(j0, min(j0 + 2, ny)) for i in range(i0, min(i0 + 2, nx))], np.int64))
    return out


def line_blocks(nx, ny, nz=1):
    """grid lines in x"""
    return [np.arange(nx, dtype=np.int64) + nx * q for q in range(ny * nz)]


def consecutive_blocks(sizes, start=0):
    out, r = [], start
    for m in sizes:
        out.append(np.arange(r, r + m, dtype=np.int64))
        r += m
    return out


def slot_offsets(blocks):
    return np.concatenate([[0], np.cumsum([len(p) for p in blocks])]).astype(np.int64)


# ---- colouring -----------------------------------------------------------------------------------------------------------
def conflicts(A: O.CSR, blocks):
    """the conflict sets: q in out[p] iff p != q and the blocks share a row or a row of one stores an entry in a column of the other"""
    n = A.n
    S = A.scipy()
    pat = sp.csr_matrix((np.ones(len(S.data)), S.indices, S.indptr), shape=S.shape)
    B = sp.csr_matrix((np.ones(sum(len(p) for p in blocks)), (np.repeat(np.arange(len(blocks)), [len(p) for p in blocks]), np.concatenate(blocks))), shape=(len(blocks), n))
    Cm = (B @ (sp.identity(n) + pat + pat.T) @ B.T).tocsr()
    return [set(Cm.indices[Cm.indptr[p]:Cm.indptr[p + 1]].tolist()) - {p} for p in range(len(blocks))]


def first_fit_colors(A: O.CSR, blocks) -> np.ndarray:
    """the stated rule: blocks in block order, the smallest colour no conflicting block before it has taken"""
    nb = conflicts(A, blocks)
    col = np.full(len(blocks), -1, np.int32)
    for p in range(len(blocks)):
        used = {int(col[q]) for q in nb[p] if col[q] >= 0}
        c = 0
        while c in used:
            c += 1
        col[p] = c
    return col


def colors_valid(A: O.CSR, blocks, colors) -> bool:
    nb = conflicts(A, blocks)
    return all(colors[q] != colors[p] for p in range(len(blocks)) for q in nb[p])


def visit_order(colors, backward=False):
    """(colour, index) order; a backward sweep takes the colours in descending order"""
    colors = np.asarray(colors)
    key = -colors if backward else colors
    return [int(p) for p in np.lexsort((np.arange(len(colors)), key))]


def directions(sweep_type):
    return (FWD, BWD) if sweep_type == SYM else (sweep_type,)


# ---- the reference -------------------------------------------------------------------------------------------------------
class Reference:
    """per block: A_PP, numpy's Cholesky factor, |A_PP^-1|, |L^-T|, kappa_2(A_PP), and the exterior rows of A"""

    def __init__(self, A: O.CSR, blocks):
        self.A, self.blocks, self.n = A, [np.asarray(p, np.int64) for p in blocks], A.n
        D = A.dense()
        self.off = slot_offsets(blocks)
        self.blk = []
        for P in self.blocks:
            App = np.tril(D[np.ix_(P, P)])
            App = App + np.tril(App, -1).T  # the lower triangle, as dpotrf('L') reads it
            L = np.linalg.cholesky(App)
            ext = D[P].copy()
            ext[:, P] = 0.0
            w = np.linalg.eigvalsh(App)
            Winv = sla.solve_triangular(L, np.eye(len(P)), lower=True)
            self.blk.append(dict(App=App, L=L, ext=ext, kappa=float(w[-1] / w[0]), absinv=np.abs(np.linalg.inv(App)), absWT=np.abs(Winv.T), W=Winv))


def ref_sweep(R: Reference, colors, b, y, xi_slots=None, backward=False, bound=False, err=None):
    """One directional sweep by the reference.  bound=True also returns e, a running bound on |y_impl - y_ref| row by row for an
    implementation that forms every r_i with a backward-stable dot product and every block solve with the forward error of
    tests/chol_edge_refs.py (fwd_bound(m, kappa_2(A_PP)) relative to max |y_P|, for the solve and for the noise term):
        e_r  = |A_ext| e + gamma(row length + 1) (|b_P| + |A_ext| |y|)
        e_P  = |A_PP^-1| e_r + fwd_bound(m, kappa_P) (max |A_PP^-1 r| + max |L^-T xi_P|)
    with e carried from block to block (err: the bound the sweep starts from).  Nothing here comes from the code under test."""
    y = np.array(y, np.float64, copy=True)
    e = np.zeros(R.n) if err is None else np.array(err, copy=True)
    for p in visit_order(colors, backward):
        P, K = R.blocks[p], R.blk[p]
        r = b[P] - K["ext"] @ y
        v = sla.solve_triangular(K["L"], r, lower=True)
        if xi_slots is not None:
            v = v + xi_slots[R.off[p]:R.off[p + 1]]
        new = sla.solve_triangular(K["L"].T, v, lower=False)
        if bound:
            aext = np.abs(K["ext"])
            er = aext @ e + gamma(int((K["ext"] != 0).sum(axis=1).max()) + 1) * (np.abs(b[P]) + aext @ np.abs(y))
            det = np.abs(sla.solve_triangular(K["L"].T, sla.solve_triangular(K["L"], r, lower=True), lower=False)).max()
            noi = 0.0 if xi_slots is None else np.abs(sla.solve_triangular(K["L"].T, xi_slots[R.off[p]:R.off[p + 1]], lower=False)).max()
            e[P] = K["absinv"] @ er + fwd_bound(len(P), K["kappa"]) * (det + noi)
        y[P] = new
    return (y, e) if bound else y


def ref_apply(R, colors, b, y, sweep_type=FWD, xi_fn=None, bound=False):
    """one sample of `sweep_type`; xi_fn(d) gives the slot normals of directional sweep d (None: deterministic)"""
    e = None
    for d, dr in enumerate(directions(sweep_type)):
        out = ref_sweep(R, colors, b, y, None if xi_fn is None else xi_fn(d), dr == BWD, bound, e)
        y, e = out if bound else (out, None)
    return (y, e) if bound else y


def ref_maps(R: Reference, colors, sweep_type):
    """(G, N) of y <- G y + N xi + (...) b for one sample of `sweep_type`: columns from unit vectors through ref_sweep"""
    n, ns = R.n, int(R.off[-1])
    z = np.zeros(n)

    def one(backward):
        G = np.column_stack([ref_sweep(R, colors, z, np.eye(n)[:, j], None, backward) for j in range(n)])
        N = np.column_stack([ref_sweep(R, colors, z, z, np.eye(ns)[:, s], backward) for s in range(ns)])
        return G, N

    if sweep_type != SYM:
        return one(sweep_type == BWD)
    (Gf, Nf), (Gb, Nb) = one(False), one(True)
    return Gb @ Gf, np.hstack([Gb @ Nf, Nb])


def covariance_error(A: O.CSR, G, N) -> float:
    """||S - A^-1||_F / ||A^-1||_F for the stationary covariance S of (G, N): the metric of the reference's src/stats.c"""
    Q = np.linalg.inv(A.dense())
    return float(np.linalg.norm(O.stationary_covariance(G, N) - Q) / np.linalg.norm(Q))


# ---- the walk-through ----------------------------------------------------------------------------------------------------
def gram(W):
    """M = W^T W as pmg_blockgibbs_host.c forms it: M_ij = sum_k W_ki W_kj, k ascending from zero, two roundings per term"""
    m = W.shape[0]
    M = np.zeros((m, m))
    for k in range(m):
        M = M + np.outer(W[k], W[k])
    return M


def walk_sweep(A: O.CSR, blocks, colors, Ws, b, y, xi_slots=None, backward=False, pos=None):
    """one directional sweep in the kernel's order of operations; b, y indexed by position pos[row] (None: by row).  The blocks
    of a colour do not read each other's rows, so visiting them one after the other equals the launch."""
    y = np.array(y, np.float64, copy=True)
    pos = np.arange(A.n) if pos is None else np.asarray(pos)
    off = slot_offsets(blocks)
    rp, ci, va = A.rowptr, A.colidx, A.vals
    for p in visit_order(colors, backward):
        P, W = np.asarray(blocks[p]), Ws[p]
        m = len(P)
        inblk = set(P.tolist())
        r = np.zeros(m)
        for i, row in enumerate(P):
            s = b[pos[row]]
            for k in range(rp[row], rp[row + 1]):
                if int(ci[k]) not in inblk:
                    s = s - va[k] * y[pos[ci[k]]]
            r[i] = s
        M = gram(W)
        out = np.zeros(m)
        for j in range(m):
            out = out + M[:, j] * r[j]
        if xi_slots is not None:
            xi, acc = xi_slots[off[p]:off[p + 1]], np.zeros(m)
            for j in range(m):
                acc = acc + W[j, :] * xi[j]
            out = out + acc
        y[pos[P]] = out
    return y


def walk_apply(A, blocks, colors, Ws, b, y, sweep_type=FWD, xi_fn=None, pos=None):
    for d, dr in enumerate(directions(sweep_type)):
        y = walk_sweep(A, blocks, colors, Ws, b, y, None if xi_fn is None else xi_fn(d), dr == BWD, pos)
    return y


def noise_bound(A: O.CSR, blocks, colors, Ws, sweep_type, nsamples, tol, y_scale, b_scale, xi_scale):
    """|y_dev - y_fed| row by row after `nsamples` samples, for two chains that run the same operations, one on normals the
    device draws and one on the oracle's, every pair of normals within `tol` of each other.  The difference obeys the sweep's
    own linear map, so it is carried EXACTLY: E (rows x injected normals) through  E_P <- M (-A_ext E), E[P, slots of this
    sweep] += W^T  per block update, and |delta y| <= (|E| 1) tol -- the term |W^T| tol propagated through the sweeps.  The
    two chains also round differently once their inputs differ: every update of a row may differ by twice its rounding error,
    2 gamma(m + row length + 2) (||M||_inf (b_scale + ||A_ext||_inf y_scale) + ||W^T||_inf xi_scale), injected into a second
    matrix F the same way (identity in place of W^T) and summed in absolute value."""
    D = A.dense()
    off = slot_offsets(blocks)
    ns = int(off[-1])
    ndraw = nsamples * len(directions(sweep_type))
    E, F = np.zeros((A.n, ns * ndraw)), np.zeros((A.n, ns * ndraw))
    unit = np.zeros(ns * ndraw)
    d = 0
    for _ in range(nsamples):
        for dr in directions(sweep_type):
            for p in visit_order(colors, dr == BWD):
                P, W = np.asarray(blocks[p]), Ws[p]
                M = gram(W)
                ext = D[P].copy()
                ext[:, P] = 0.0
                cols = slice(d * ns + int(off[p]), d * ns + int(off[p + 1]))
                EP, FP = -M @ (ext @ E), -M @ (ext @ F)
                EP[:, cols] += W.T
                FP[:, cols] += np.eye(len(P))
                E[P], F[P] = EP, FP
                rowlen = int((ext != 0).sum(axis=1).max())
                unit[cols] = 2 * gamma(len(P) + rowlen + 2) * (np.abs(M).sum(axis=1).max() * (b_scale + np.abs(ext).sum(axis=1).max() * y_scale) + np.abs(W.T).sum(axis=1).max() * xi_scale)
            d += 1
    return np.abs(E).sum(axis=1) * tol + np.abs(F) @ unit


__all__ = [n for n in dir() if not n.startswith("_")]
assert U == 2.0**-53
