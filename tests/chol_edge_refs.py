"""High-precision references and error bounds for the dense Cholesky coarse sampler (pmg_chol.c + kernels_dense.hip).

Shared by tests/test_chol_edges.py (CPU: the references themselves) and tests/test_gpu_chol_edges.py (the device
against them).  u = 2^-53, kappa = kappa_2(A) from eigvalsh.

  factor   e_f = ||A - L L^T||_F / ||A||_F  <=  gamma_{n+1} trace(A) / ||A||_F   (classical Cholesky backward bound)
  solve    ||x - x*||_inf / ||x*||_inf      <=  C_FWD n kappa u
  sample   ||y - y*||_inf / ||y*||_inf      <=  C_FWD n kappa u
  noise    ||L_dev^T z - xi||_2 / ||xi||_2   <=  C_FWD n sqrt(kappa) u,  z = noisy - deterministic sample, same b

with C_FWD = 8.  The noise check is the vector form of |(||L^T z|| - ||xi||)| / ||xi||, which it implies.  e_f is evaluated in
long double from the exact double entries of A and L up to n = LD_FULL_MAX; above that the Frobenius norm of A - L L^T is
estimated from PROBES random probes v (E ||E v||^2 = ||E||_F^2 for v ~ N(0, I)), with A v - L (L^T v) in long double.
"""
from __future__ import annotations

import mpmath
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import oracle as O

U = 2.0**-53
C_FWD = 8
LD = np.longdouble
LD_FULL_MAX = 1025
PROBES = 4
MP_MAX = 97  # largest n with the mpmath sample reference


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


def dense_spd(n: int, kappa: float, seed: int) -> np.ndarray:
    """Q diag(lambda) Q^T, Q Haar-random, lambda log-spaced over [1, kappa]; exactly symmetric"""
    rng = np.random.default_rng(seed)
    Q, R = np.linalg.qr(rng.standard_normal((n, n)))
    Q = Q * np.sign(np.diag(R))
    A = (Q * np.geomspace(1.0, kappa, n)) @ Q.T
    return (A + A.T) * 0.5


def to_csr(M):
    """(rowptr, colidx, vals) of every stored entry of a dense or sparse matrix; explicit entries of a dense matrix are all
    of its non-zeros (NaN included)"""
    m = M.tocsr() if sp.issparse(M) else sp.csr_matrix(M)
    m.sort_indices()
    return m.indptr.astype(np.int32), m.indices.astype(np.int32), np.ascontiguousarray(m.data, np.float64)


def lowrank_sum(A: np.ndarray, B: np.ndarray, S: np.ndarray) -> np.ndarray:
    """A + B diag(S) B^T, accumulated rank by rank as PCSetUp_CholSampler's MATLRC branch does"""
    P = np.array(A, dtype=np.float64, copy=True)
    for c in range(B.shape[1]):
        P += np.outer(B[:, c], S[c] * B[:, c])
    return P


def ld_mul(M: np.ndarray, X: np.ndarray, rows: int = 512) -> np.ndarray:
    """M X in long double, M converted a block of rows at a time"""
    X = np.asarray(X).astype(LD)
    out = np.empty((M.shape[0],) + X.shape[1:], LD)
    for r0 in range(0, M.shape[0], rows):
        out[r0 : r0 + rows] = M[r0 : r0 + rows].astype(LD) @ X
    return out


def eig_range(A: np.ndarray):
    w = np.linalg.eigvalsh(A)
    assert w[0] > 0, "test matrix is not SPD"
    return float(w[0]), float(w[-1])


def factor_error(A: np.ndarray, L: np.ndarray, seed: int = 0) -> float:
    n = A.shape[0]
    nA = np.sqrt(np.sum(A.astype(LD) ** 2))
    if n <= LD_FULL_MAX:
        Ll = L.astype(LD)
        return float(np.sqrt(np.sum((A.astype(LD) - Ll @ Ll.T) ** 2)) / nA)
    V = np.random.default_rng(seed).standard_normal((n, PROBES))
    R = ld_mul(A, V) - ld_mul(L, ld_mul(L.T, V))
    return float(np.sqrt(np.sum(R**2) / PROBES) / nA)


def factor_bound(A: np.ndarray) -> float:
    return gamma(A.shape[0] + 1) * float(np.trace(A)) / float(np.linalg.norm(A))


def fwd_bound(n: int, kappa: float) -> float:
    return C_FWD * n * kappa * U


def noise_bound(n: int, kappa: float) -> float:
    return C_FWD * n * np.sqrt(kappa) * U


def rel_inf(y: np.ndarray, ref: np.ndarray) -> float:
    return float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))


def solve_ref(A: np.ndarray, b: np.ndarray, steps: int = 2) -> np.ndarray:
    """x* = A^-1 b: float64 LU solve + `steps` refinement steps with the residual in long double"""
    lu = sla.lu_factor(A)
    x = sla.lu_solve(lu, b)
    for _ in range(steps):
        r = b.astype(LD) - ld_mul(A, x)
        x = x + sla.lu_solve(lu, r.astype(np.float64))
    return x


def mp_sample(A: np.ndarray, b: np.ndarray, xi, dps: int = 40) -> np.ndarray:
    """y* = L*^-T (L*^-1 b + xi) with L* the Cholesky factor of the exact double entries of A in mpmath at `dps` digits;
    xi = None gives A^-1 b"""
    n = A.shape[0]
    with mpmath.workdps(dps):
        a = [[mpmath.mpf(float(A[i, j])) for j in range(i + 1)] for i in range(n)]
        L = [[mpmath.mpf(0)] * (i + 1) for i in range(n)]
        for j in range(n):
            d = a[j][j] - mpmath.fsum(L[j][k] ** 2 for k in range(j))
            assert d > 0
            L[j][j] = mpmath.sqrt(d)
            for i in range(j + 1, n):
                L[i][j] = (a[i][j] - mpmath.fsum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
        v = [mpmath.mpf(0)] * n
        for i in range(n):
            v[i] = (mpmath.mpf(float(b[i])) - mpmath.fsum(L[i][k] * v[k] for k in range(i))) / L[i][i]
        if xi is not None:
            v = [v[i] + mpmath.mpf(float(xi[i])) for i in range(n)]
        y = [mpmath.mpf(0)] * n
        for i in reversed(range(n)):
            y[i] = (v[i] - mpmath.fsum(L[k][i] * y[k] for k in range(i + 1, n))) / L[i][i]
        return np.array([float(t) for t in y])


def sample_ref(A: np.ndarray, b: np.ndarray, xi: np.ndarray, L_ref=None) -> np.ndarray:
    """the noisy-sample reference: mpmath up to MP_MAX rows, the oracle's y = L^-T (L^-1 b + xi) above (L_ref: LAPACK's
    factor, else the oracle's potrf)"""
    if A.shape[0] <= MP_MAX:
        return mp_sample(A, b, xi)
    return O.chol_sample(O.potrf_lower(A) if L_ref is None else L_ref, b, xi)


def noise_error(L: np.ndarray, z: np.ndarray, xi: np.ndarray) -> float:
    r = ld_mul(L.T, z) - xi.astype(LD)
    return float(np.sqrt(np.sum(r**2)) / np.sqrt(np.sum(xi.astype(LD) ** 2)))


def with_failing_minor(A: np.ndarray, m: int) -> np.ndarray:
    """A with A[m-1, m-1] := sum_{k < m-1} L[m-1, k]^2 - A[m-1, m-1] / 2 (L = LAPACK's factor of A): the pivot of order m is
    -A[m-1, m-1] / 2, every smaller leading minor is A's"""
    L = np.linalg.cholesky(A)
    i = m - 1
    B = np.array(A, copy=True)
    B[i, i] = float(np.sum(L[i, :i] ** 2)) - 0.5 * A[i, i]
    return B


def lapack_info(A: np.ndarray) -> int:
    """dpotrf('L')'s info: 0 or the order of the first leading minor that is not positive definite"""
    return int(sla.lapack.dpotrf(np.tril(A), lower=1, clean=0)[1])
