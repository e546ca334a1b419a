"""Cases, inputs, extended-precision reference and error bounds for the Woodbury term (pmg_woodbury.c on kernels_lrc.hip and
kernels_lrc_chains.hip), and the chain counts that reach every lane split of the chain kernels.  Importable without a device;
tests/test_woodbury_cases.py checks this module on the CPU, tests/test_gpu_woodbury_term.py and
tests/test_gpu_chain_lane_splits.py run the library against it.

Inputs, deterministic from (n, k, seed): column j of B has max(1, n // 3) random rows with entries uniform(0.5, 1.5) /
sqrt(n // 3 or 1); the "solver result" is C = B / d[:, None] with d = uniform(2, 6, n); S = uniform(20, 90, k).  Flags:
  mixed  random row signs on B and S[1::2] < 0 (sqrt|S| of a negative S);
  perm   the columns of C rotated by one: T is unsymmetric, its diagonal is not its largest entry, the Gauss-Jordan inverse
         has to pivot;
  pad    B is handed over with ldb = n + 3, the pad rows NaN.
reference() asserts cond(T_ref) <= COND_CAP for every case: a condition on the inputs, not a tolerance.

Reference (np.longdouble, eps < 2e-19 asserted): T = S^-1 + B^T C; G = C T^-1 with the float64 inverse polished by three
Newton steps in extended precision; w = b + B (sqrt|S| o xi), xi = oracle.noise_rows(k, seed, counter);
y' = y - G (B^T y).

Bounds, each per entry and computed from the reference; u = 2^-53, gamma(m) = m u / (1 - m u):
  B^T y       |dt_j| <= gamma(64) sum_r |B_rj y_r|.  The kernels' order puts a term through 16 fma (4096 rows of a block over
              256 threads), 6 shuffle and 2 block additions, then ceil(nb / 64) + 6 additions of the block sums: under 64 for
              n below 8 million rows.  (gamma(n) is the order-free fallback should a kernel change alter the order.)
  correction  |dy'_r| <= gamma(k + 2) (|y_r| + sum_j |G_rj t_j|) + sum_j |G_rj| dt_j.  The GPU test holds the device result to
              it twice: with the reference's G, and with the G the handle holds (pmg_woodbury_get_correction), which keeps
              the error G itself is allowed below out of this bound.
  noisy rhs   |dw_r| <= gamma(k + 2) (|b_r| + sum_j |B_rj c_j|) + sum_j |B_rj| sqrt|S_j| NORMAL_TOL, c = sqrt|S| o xi;
              NORMAL_TOL = 1e-13 is the project's tolerance for the device normals against the oracle's (test_gpu_mcsor.py).
  G           |dG_rj| <= G_MARGIN k u cond(T_ref) max|G_ref|.  The floor k u cond max|G| is what a backward-stable inverse
              costs; numpy's float64 C @ inv(T) measures 0.004 to 2.6 of it on the cases below.  G_MARGIN is the one measured
              number here: 4 times the largest ratio the library's Gauss-Jordan inverse + lrc_gemm_small_kernel showed on an
              MI355X, rounded up to a power of two (at most 64: a larger ratio would be a finding, not a margin).

Measured ratios |G_dev - G_ref|.max() / floor per case (G_RATIOS_MEASURED below repeats them for the tests):
  n1-k1 0.735, n1-k2-pad 0.0872, n63-k1-pad 1.22, n63-k5-perm 0.0575, n63-k9-mixed 0.0362, n257-k2 0.478,
  n257-k8-mixed-perm-pad 0.0551, n257-k33 0.00708, n4095-k4-perm 0.154, n4095-k63-mixed 0.00466, n4096-k5-pad 0.271,
  n4096-k64 0.00648, n4097-k4-mixed-pad 0.224, n4097-k9-perm 0.0745, n4097-k33 0.018, n8193-k8-pad 0.115,
  n8193-k63-perm 0.00544, n8193-k64 0.00577, n8193-k64-mixed-perm 0.00463, n262145-k5-mixed-pad 0.175, n262145-k9-perm 0.0986.
The largest, 1.22, is k = 1 at cond 1: three roundings of a scalar.  G_MARGIN = 4 * 1.22 rounded up to a power of two = 8.
"""
from __future__ import annotations

import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

import oracle as O

L = np.longdouble
U = 2.0**-53
NORMAL_TOL = 1e-13
COND_CAP = 1e3
MASK64 = 0xFFFFFFFFFFFFFFFF

# the kernels' constants, restated (tests/test_woodbury_cases.py reads them out of the .hip sources)
DENSE_ROWS_PER_BLOCK = 4096  # lrc_btx_partial_kernel, lrc_btx_chains_kernel<16, false, *>
COMPACT_ROWS_PER_BLOCK = 1024  # lrc_btx_rows_partial_kernel, lrc_btx_chains_kernel<4, true, *>, lrc_small_chains_kernel
KB = 4  # columns of B^T y per pass of the chain kernels
REDUCE_LANES = 64  # lrc_reduce_kernel: lane l adds the blocks l, l + 64, ...
BTX_DEPTH = 64  # the additions a term of B^T y can pass through, see above

Case = namedtuple("Case", "n k mixed perm pad")
KS = [1, 2, 4, 5, 8, 9, 33, 63, 64]
NS = [1, 63, 257, 4095, 4096, 4097, 8193]
N_WRAP = 262145  # 65 blocks of 4096 rows: the reduce lanes wrap
CASES = [
    Case(1, 1, False, False, False),
    Case(1, 2, False, False, True),
    Case(63, 1, False, False, True),
    Case(63, 5, False, True, False),
    Case(63, 9, True, False, False),
    Case(257, 2, False, False, False),
    Case(257, 8, True, True, True),
    Case(257, 33, False, False, False),
    Case(4095, 4, False, True, False),
    Case(4095, 63, True, False, False),
    Case(4096, 5, False, False, True),
    Case(4096, 64, False, False, False),
    Case(4097, 4, True, False, True),
    Case(4097, 9, False, True, False),
    Case(4097, 33, False, False, False),
    Case(8193, 8, False, False, True),
    Case(8193, 63, False, True, False),
    Case(8193, 64, False, False, False),
    Case(8193, 64, True, True, False),
    Case(N_WRAP, 5, True, False, True),
    Case(N_WRAP, 9, False, True, False),
]

# |G_dev - G_ref|.max() / (k u cond(T_ref) max|G_ref|) on an MI355X, per case; G_MARGIN = 4 max, rounded up to a power of two
G_RATIOS_MEASURED = {
    "n1-k1": 0.735,
    "n1-k2-pad": 0.0872,
    "n63-k1-pad": 1.22,
    "n63-k5-perm": 0.0575,
    "n63-k9-mixed": 0.0362,
    "n257-k2": 0.478,
    "n257-k8-mixed-perm-pad": 0.0551,
    "n257-k33": 0.00708,
    "n4095-k4-perm": 0.154,
    "n4095-k63-mixed": 0.00466,
    "n4096-k5-pad": 0.271,
    "n4096-k64": 0.00648,
    "n4097-k4-mixed-pad": 0.224,
    "n4097-k9-perm": 0.0745,
    "n4097-k33": 0.018,
    "n8193-k8-pad": 0.115,
    "n8193-k63-perm": 0.00544,
    "n8193-k64": 0.00577,
    "n8193-k64-mixed-perm": 0.00463,
    "n262145-k5-mixed-pad": 0.175,
    "n262145-k9-perm": 0.0986,
}
G_MARGIN = 8.0  # 4 * 1.22 = 4.88

# ---- chain counts: LPRL = log2 of the lanes per chain group (the count rounded up to a power of two, at most 64), the chunks
# of 64 chains (blockIdx.y) and the live lanes of the last chunk
CHAINS = [2, 4, 9, 16, 17, 33, 63, 64, 128, 129]
CONTROLS = [1, 3, 8, 32, 65]
CHAIN_TABLE = {
    # C: (LPRL, chunks, live lanes in the last chunk)
    1: (0, 1, 1),
    2: (1, 1, 2),
    3: (2, 1, 3),
    4: (2, 1, 4),
    8: (3, 1, 8),
    9: (4, 1, 9),
    16: (4, 1, 16),
    17: (5, 1, 17),
    32: (5, 1, 32),
    33: (6, 1, 33),
    63: (6, 1, 63),
    64: (6, 1, 64),
    65: (6, 2, 1),
    128: (6, 2, 64),
    129: (6, 3, 1),
}
# the chains-against-single-chain shapes: below and above one block of 4096 rows, k on both sides of KB, odd, and 64
CHAIN_SHAPES = [(257, 1), (257, 4), (257, 5), (257, 64), (4097, 1), (4097, 4), (4097, 5), (4097, 64)]
CHAIN_WRAP_SHAPE, CHAIN_WRAP_COUNTS = (N_WRAP, 5), [2, 16, 65]


def lane_split(C: int):
    """(LPRL, chunks, live lanes in the last chunk) as lpr_log2_of / chunks_of of kernels_lrc_chains.hip give them"""
    lprl = 0
    while lprl < 6 and (1 << lprl) < C:
        lprl += 1
    chunks = (C + 63) // 64
    return lprl, chunks, C - 64 * (chunks - 1)


def chain_seeds(count: int) -> list[int]:
    """full 64-bit seeds; a prefix of a longer list is the shorter list"""
    return [((0x9E3779B97F4A7C15 * (c + 1)) ^ 0xD6E8FEB86659FD93) & MASK64 for c in range(count)]


def chain_case(n: int, k: int) -> Case:
    """the inputs of a chains-against-single-chain shape: mixed signs above one block; the 65-block shape is the tabled case"""
    if n == N_WRAP:
        return next(c for c in CASES if (c.n, c.k) == (n, k))
    return Case(n, k, n > DENSE_ROWS_PER_BLOCK, False, False)


def case_id(c: Case) -> str:
    return f"n{c.n}-k{c.k}" + "".join("-" + f for f in ("mixed", "perm", "pad") if getattr(c, f))


def gamma(m: int) -> float:
    return m * U / (1.0 - m * U)


def _rng_seed(c: Case) -> int:
    return 1000003 * c.n + 101 * c.k + 4 * c.mixed + 2 * c.perm + c.pad


def noise_key(c: Case):
    """(seed, counter) of the case's noisy right-hand side: full 64-bit values with high words set"""
    s = _rng_seed(c)
    return (0xD1B54A32D192ED03 * (s + 1)) & MASK64 | (1 << 63), (0xC2B2AE3D27D4EB4F ^ (s << 17)) & MASK64 | (1 << 62)


@functools.lru_cache(maxsize=None)
def inputs(c: Case) -> SimpleNamespace:
    """B, C (n x k float64), S (k), the host image of B (ldb x k, column-major, pad rows NaN), b and y (n)"""
    n, k = c.n, c.k
    rng = np.random.default_rng(_rng_seed(c))
    m = max(1, n // 3)
    B = np.zeros((n, k))
    for j in range(k):
        idx = rng.choice(n, size=m, replace=False)
        B[idx, j] = rng.uniform(0.5, 1.5, m) / np.sqrt(n // 3 or 1)
    d = rng.uniform(2.0, 6.0, n)
    S = rng.uniform(20.0, 90.0, k)
    if c.mixed:
        B *= rng.choice([-1.0, 1.0], n)[:, None]
        S[1::2] *= -1.0
    Cm = B / d[:, None]
    if c.perm:
        Cm = np.roll(Cm, 1, axis=1)
    ldb = n + 3 if c.pad else n
    B_host = np.full((ldb, k), np.nan, order="F")
    B_host[:n] = B
    b, y = rng.standard_normal(n), rng.standard_normal(n)
    for a in (B, Cm, S, B_host, b, y):
        a.setflags(write=False)
    return SimpleNamespace(n=n, k=k, B=B, C=Cm, S=S, ldb=ldb, B_host=B_host, b=b, y=y)


def _ext(a):
    assert np.finfo(L).eps < 2e-19, f"np.longdouble is not an extended format here (eps = {np.finfo(L).eps})"
    return np.asarray(a, dtype=L)


def _inverse_ext(T):
    """the float64 inverse, polished by three Newton steps X <- X + X (I - T X) in extended precision"""
    X = _ext(np.linalg.inv(np.asarray(T, np.float64)))
    eye = np.eye(len(T), dtype=L)
    for _ in range(3):
        X = X + X @ (eye - T @ X)
    return X


def build(B, Cm, S) -> SimpleNamespace:
    """T = S^-1 + B^T C, T^-1, G = C T^-1 and cond(T) in extended precision"""
    Bx, Cx, Sx = _ext(B), _ext(Cm), _ext(S)
    T = Bx.T @ Cx + np.diag(L(1) / Sx)
    Tinv = _inverse_ext(T)
    cond = float(np.linalg.cond(np.asarray(T, np.float64)))
    return SimpleNamespace(B=Bx, S=Sx, T=T, Tinv=Tinv, G=Cx @ Tinv, cond=cond)


@functools.lru_cache(maxsize=None)
def reference(c: Case) -> SimpleNamespace:
    I = inputs(c)
    R = build(I.B, I.C, I.S)
    assert R.cond <= COND_CAP, (case_id(c), R.cond)
    return R


def g_floor(R) -> float:
    """k u cond(T_ref) max|G_ref|: what a backward-stable inverse costs an entry of G"""
    return len(R.S) * U * R.cond * float(np.abs(R.G).max())


def g_ratio(G_got, R) -> float:
    return float(np.abs(_ext(G_got) - R.G).max()) / g_floor(R)


def noisy_rhs_ref(R, b, seed: int, counter: int, S=None):
    """(w, bound): w = b + B (sqrt|S| o xi) with the oracle's normals of the row stream (seed, counter)"""
    k = R.B.shape[1]
    xi = _ext(O.noise_rows(k, seed, counter))
    sq = np.sqrt(np.abs(R.S if S is None else _ext(S)))
    c = sq * xi
    bx = _ext(b)
    w = bx + R.B @ c
    aB = np.abs(R.B)
    bound = gamma(k + 2) * (np.abs(bx) + aB @ np.abs(c)) + (aB @ sq) * L(NORMAL_TOL)
    return w, bound


def btx_ref(R, y, drop_row=None):
    """(t, dt): t = B^T y and its bound; drop_row leaves that row out of the sums (the negative control)"""
    yx = _ext(y).copy()
    if drop_row is not None:
        yx[drop_row] = 0
    return R.B.T @ yx, gamma(BTX_DEPTH) * (np.abs(R.B).T @ np.abs(yx))


def correct_ref(R, y, G=None, drop_row=None):
    """(y', bound): y' = y - G (B^T y), G = the reference's or the given one (the matrix the call under test applies)"""
    k = R.B.shape[1]
    Gx = R.G if G is None else _ext(G)
    t, dt = btx_ref(R, y, drop_row)
    yx = _ext(y)
    aG = np.abs(Gx)
    return yx - Gx @ t, gamma(k + 2) * (np.abs(yx) + aG @ np.abs(t)) + aG @ dt


def heaviest_row(R, y) -> int:
    """the row whose term B_r0 y_r of B^T y is largest: the one the negative control leaves out"""
    return int(np.argmax(np.abs(np.asarray(R.B[:, 0], np.float64) * y)))


def excess(got, ref, bound) -> float:
    """max over the entries of |got - ref| / bound (inf where got is not finite): within the bound iff <= 1"""
    got = np.asarray(got)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(_ext(got) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, L(0), err / bound)
    return float(q.max()) if q.size else 0.0


def float64_evaluation(I, seed: int, counter: int, S=None, drop_row=None) -> SimpleNamespace:
    """the same formulas in plain float64 numpy: the stand-in for the device on the CPU"""
    S = I.S if S is None else S
    T = I.B.T @ I.C + np.diag(1.0 / S)
    G = I.C @ np.linalg.inv(T)
    w = I.b + I.B @ (np.sqrt(np.abs(S)) * O.noise_rows(I.k, seed, counter))
    y = I.y.copy()
    if drop_row is not None:
        y[drop_row] = 0.0
    return SimpleNamespace(G=G, w=w, y=I.y - G @ (I.B.T @ y))
