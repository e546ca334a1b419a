"""Wide-row and irregular workloads for the AIJ path (sliced-ELL sweeps, CSR transfers, dense coarse sampler).  Helpers only.

Every hierarchy of the other AIJ tests comes from plain aggregation: one entry per row of P, operator rows of at most ~27
entries.  The reference's benchmark runs smoothed aggregation instead (`-pc_gamgmc_mg_type gamg`,
`-gamgmc_pc_gamg_agg_nsmooths 2`), whose levels have rows of hundreds of entries and whose P^T has rows of thousands.  Those
are built here with numpy / scipy, deterministically, together with single-level matrices whose structure is awkward for the
sliced-ELL layout: hub rows, a dense clique, empty slices, stored zeros, unsorted rows, colour sizes around the 64-row slice and a
scrambled numbering that makes the set-up take the breadth-first layout.  All matrices are symmetric, strictly diagonally
dominant with a positive diagonal, hence SPD."""
from pathlib import Path

import numpy as np
import scipy.sparse as sp

import oracle as O
from parmgmc_amd.unstructured import assemble_p1, greedy_aggregation, read_gmsh41_triangles, refine_uniform

MESH = Path(__file__).resolve().parent / "golden" / "lshape.msh"
COARSE_MAX = 500  # 25^3 stops at 179 rows, 129^2 at 25, lshape refined 3 times at 408


def _csr(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


def smoothed_aggregation(A, nsmooth, coarse_max=COARSE_MAX, max_levels=12):
    """(operators, interpolations) for MGMC.from_hierarchy, level 0 = coarsest.  Tentative P from greedy_aggregation, then
    `nsmooth` Jacobi steps P <- (I - w D^-1 A) P with w = 4 / (3 rho), rho the Gershgorin bound of D^-1 A; A_c = P^T A P."""
    ops, ps = [_csr(A)], []
    while ops[-1].shape[0] > coarse_max and len(ops) < max_levels:
        Af = ops[-1]
        P = greedy_aggregation(Af)
        d = Af.diagonal()
        rho = (abs(Af).sum(axis=1).A1 / np.abs(d)).max()
        DinvA = _csr(sp.diags(1.0 / d) @ Af)
        for _ in range(nsmooth):
            P = _csr(P - (4.0 / (3.0 * rho)) * (DinvA @ P))
        ps.append(P)
        ops.append(_csr(P.T @ Af @ P))
    ops, ps = ops[::-1], ps[::-1]
    operators = [(m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data) for m in ops]
    interpolations = [None] + [(p.indptr.astype(np.int32), p.indices.astype(np.int32), p.data) for p in ps]
    return operators, interpolations


def _lshape(refine):
    xy, tris = read_gmsh41_triangles(MESH)
    for _ in range(refine):
        xy, tris = refine_uniform(xy, tris)
    return assemble_p1(xy, tris, 1.0)


def hierarchy(name):
    """the smoothed-aggregation hierarchies: 'sa3d25' (7-point 25^3, nsmooth 2), 'sa2d129' (5-point 129^2, nsmooth 2),
    'salshape' (P1 on lshape.msh refined 3 times, nsmooth 2)"""
    if name == "sa3d25":
        return smoothed_aggregation(O.shifted_laplace(25, 25, 25, 1.0).scipy(), 2)
    if name == "sa2d129":
        return smoothed_aggregation(O.shifted_laplace(129, 129, 1, 1.0).scipy(), 2)
    if name == "salshape":
        return smoothed_aggregation(_lshape(3), 2)
    raise KeyError(name)


HIERARCHIES = ["sa3d25", "sa2d129", "salshape"]


def as_scipy(triple, shape):
    rp, ci, v = triple
    return sp.csr_matrix((v, ci, rp), shape=shape)


# --- single-level matrices -------------------------------------------------------------------------------------------------
def _spd_from_offdiag(rows, cols, vals, n):
    """symmetric off-diagonal part from one triangle's (rows, cols, vals), diagonal = row sum of |offdiag| + 1"""
    M = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    M.sum_duplicates()
    M = M + M.T
    M = M + sp.diags(np.abs(M).sum(axis=1).A1 + 1.0)
    return _csr(M)


def _lap2d(nx, ny):
    return O.shifted_laplace(nx, ny, 1, 1.0).scipy()


HUB_ROWS = (37, 2100, 4000)  # of the 64 x 64 grid: rank 0 of two owns the first, rank 1 the others
HUB_DEGREES = (1000, 3000, 100)


def hubs():
    """64 x 64 Laplacian whose rows 37, 2100 and 4000 are coupled to 1000, 3000 and 100 random rows"""
    rng = np.random.default_rng(1)
    L = sp.coo_matrix(sp.triu(_lap2d(64, 64), 1))
    r, c, v = [L.row], [L.col], [L.data]
    for h, k in zip(HUB_ROWS, HUB_DEGREES):
        nb = rng.choice(np.setdiff1d(np.arange(4096), [h]), k, replace=False)
        r.append(np.full(k, h)), c.append(nb), v.append(-rng.uniform(0.05, 0.5, k))
    return _spd_from_offdiag(np.concatenate(r), np.concatenate(c), np.concatenate(v), 4096)


def clique():
    """1-D Laplacian of 900 rows with rows 400..439 coupled to each other: at least 40 colours"""
    rng = np.random.default_rng(2)
    n = 900
    r, c = np.triu_indices(40, 1)
    rows = np.concatenate([np.arange(n - 1), 400 + r])
    cols = np.concatenate([np.arange(1, n), 400 + c])
    return _spd_from_offdiag(rows, cols, -rng.uniform(0.1, 1.0, len(rows)), n)


def isolated():
    """rows 0..255 and 700..899 diagonal-only (whole slices of width 0), the others sparse with a few rows of 150 entries"""
    rng = np.random.default_rng(3)
    n = 900
    live = np.arange(256, 700)
    r, c = [], []
    for i in live:  # a random sparse band plus far couplings
        k = 150 if i % 97 == 0 else 3
        nb = rng.choice(live, k, replace=False)
        r.append(np.full(k, i)), c.append(nb)
    r, c = np.concatenate(r), np.concatenate(c)
    keep = r != c
    return _spd_from_offdiag(r[keep], c[keep], -rng.uniform(0.1, 1.0, keep.sum()), n)


def zeros():
    """48 x 40 Laplacian plus a symmetric set of explicitly stored zeros (rows 5, 777 and 1900 widened by 60 of them)"""
    rng = np.random.default_rng(4)
    L = _lap2d(48, 40)
    n = L.shape[0]
    r = np.concatenate([rng.integers(0, n, 400), np.repeat([5, 777, 1900], 60)])
    c = np.concatenate([rng.integers(0, n, 400), rng.integers(0, n, 180)])
    r, c = np.concatenate([r, c]), np.concatenate([c, r])  # symmetric pattern
    Lc = sp.coo_matrix(L)
    rows, cols = np.concatenate([Lc.row, r]), np.concatenate([Lc.col, c])
    vals = np.concatenate([Lc.data, np.zeros(len(r))])
    # one entry per position; a position of L keeps L's value (L comes first, np.unique returns the first index)
    _, first = np.unique(rows.astype(np.int64) * n + cols, return_index=True)
    rows, cols, vals = rows[first], cols[first], vals[first]  # sorted by (row, column)
    indptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    return O.CSR(indptr, cols.astype(np.int32), vals)


def unsorted():
    """a random SPD matrix whose rows are stored in shuffled column order with the diagonal in the middle (built directly:
    O.CSR.from_scipy would sort them)"""
    rng = np.random.default_rng(5)
    n = 700
    r = np.concatenate([rng.integers(0, n, 5000), np.repeat([3, 350], 120)])
    c = np.concatenate([rng.integers(0, n, 5000), rng.integers(0, n, 240)])
    keep = r != c
    M = _spd_from_offdiag(r[keep], c[keep], -rng.uniform(0.1, 1.0, keep.sum()), n)
    rp, ci, v = [0], [], []
    for i in range(n):
        cc, vv = M.indices[M.indptr[i]:M.indptr[i + 1]], M.data[M.indptr[i]:M.indptr[i + 1]]
        off = np.flatnonzero(cc != i)
        d = np.flatnonzero(cc == i)[0]
        perm = rng.permutation(off)
        order = np.concatenate([perm[: len(perm) // 2], [d], perm[len(perm) // 2:]])
        ci.append(cc[order]), v.append(vv[order])
        rp.append(rp[-1] + len(order))
    return O.CSR(np.array(rp, np.int32), np.concatenate(ci).astype(np.int32), np.concatenate(v))


SLICE_EDGE_SIZES = (127, 128, 129, 130, 257, 258)


def tridiag(n):
    """n-row tridiagonal: two colours of ceil(n/2) and floor(n/2) rows"""
    rng = np.random.default_rng(n)
    return _spd_from_offdiag(np.arange(n - 1), np.arange(1, n), -rng.uniform(0.1, 1.0, n - 1), n)


def scrambled():
    """17 x 16 x 16 Laplacian (4352 rows) randomly renumbered, plus 3 hub rows of 200 couplings: a numbering bad enough that
    pmg_mcsor_setup lays the colours out breadth-first"""
    rng = np.random.default_rng(6)
    L = O.shifted_laplace(17, 16, 16, 1.0).scipy()
    n = L.shape[0]
    p = rng.permutation(n)
    L = sp.coo_matrix(sp.triu(L[p][:, p], 1))
    r, c, v = [L.row], [L.col], [L.data]
    for h in (11, 2222, 4321):
        nb = rng.choice(np.setdiff1d(np.arange(n), [h]), 200, replace=False)
        r.append(np.full(200, h)), c.append(nb), v.append(-rng.uniform(0.05, 0.5, 200))
    return _spd_from_offdiag(np.concatenate(r), np.concatenate(c), np.concatenate(v), n)


def irregular():
    """(name, O.CSR) of every irregular single-level matrix"""
    out = [("hubs", hubs()), ("clique", clique()), ("isolated", isolated()), ("zeros", zeros()), ("unsorted", unsorted()), ("scrambled", scrambled())]
    out += [(f"tridiag{n}", tridiag(n)) for n in SLICE_EDGE_SIZES]
    return [(name, M if isinstance(M, O.CSR) else O.CSR.from_scipy(M)) for name, M in out]


IRREGULAR = ["hubs", "clique", "isolated", "zeros", "unsorted", "scrambled"] + [f"tridiag{n}" for n in SLICE_EDGE_SIZES]


def one_sided(n, seed):
    """a random pattern with one-sided couplings (r lists c, c does not list r), diagonally dominant: the pattern on which the
    automatic colourings can give two coupled rows one colour"""
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n, 4 * n), rng.integers(0, n, 4 * n)
    keep = r != c
    M = sp.coo_matrix((-rng.uniform(0.1, 1.0, keep.sum()), (r[keep], c[keep])), shape=(n, n)).tocsr()
    M.sum_duplicates()
    M = M + sp.diags(np.abs(M).sum(axis=1).A1 + 1.0)
    return O.CSR.from_scipy(M)
