"""Launch geometry, large cases and a vectorised extended-precision reference of the Rao-Blackwellised statistics kernel
(rbstats_kernel, kernels_rbstats.hip).  Importable without a device; tests/test_rbstats_geometry_cases.py checks this module on
the CPU, tests/test_gpu_rbstats_geometry.py runs the library against it.

geometry(n, C) restates lpr_log2_of and pmgk_rbstats_geometry: lpr = C rounded up to a power of two (at most 64) lanes share a
row, a wavefront serves G = 64 / lpr rows per iteration, four wavefronts per block; more than MAXBLK = 2048 blocks' worth of rows
gives every wavefront iters > 1 iterations, and chains beyond 64 (taken in chunks of 64 by the same wavefront) cap iters at
MAXRPW = 256, the rows whose (mean, M2) a wavefront can park in LDS between chunks.

build(n, seed, integer) makes a matrix of any size without a Python loop over rows.  Row i holds LENGTHS[i % 32] off-diagonal entries;
its j-th one sits in column (i + shifts(n)[j]) mod n -- the same offset in every row, so that the matrix can be restated with
shifted copies of Y.  The kernel needs a positive finite diagonal only: the matrix is not symmetric.
  * LENGTHS differs between the two rows of every aligned pair, so row lengths vary within every group of G >= 2 consecutive
    rows; it holds 0, 1..7, exactly 8, 9..15, exactly 16 and more than 16 (the batch edges of BATCH = 8).
  * Positions 15 and 31 of LENGTHS (an empty row and a row of 19 entries) are it = 1 rows of a wavefront at every G when iters is
    2, and the period 32 is coprime to 3: test_rbstats_geometry_cases.py asserts the positions on every case.
  * Rows with i % 11 == 4 store their off-diagonal entries by descending column with the diagonal last; the others store them in
    the order of j, with the diagonal at position min(length, i % 3).
  * The offsets alternate in sign and grow from 1 to almost n / 2: a row's columns lie in other iterations of its wavefront, in
    other wavefronts and in other blocks.
integer=True: the off-diagonal value of (i, j) is INT_VALUES[(5 i + 3 j + i // 32) % 6] (int_value_index), the diagonal the power
of two at or above 1 + sum |a_ij|: with integer Y and b no operation of the contract rounds.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import rbstats_cases as R
from chainstats_cases import lpr_log2_of

BATCH = 8  # entries of a row whose loads are in flight together
MAXRPW = 256  # rows per wavefront when the chains are chunked
MAXBLK = 2048  # blocks of one launch before iters grows
WAVES = 4  # wavefronts per block


def uncapped_iters(n: int, C: int) -> int:
    rbi = WAVES * (64 >> lpr_log2_of(C))  # rows of a block per iteration
    nbi = -(-n // rbi)
    return max(1, -(-nbi // MAXBLK))


def geometry(n: int, C: int):
    """(lprl, chunks, iters, nblocks, rows_per_wavefront) of one update or cond_mean of an n x C step"""
    lprl = lpr_log2_of(C)
    G = 64 >> lprl
    nbi = -(-n // (WAVES * G))
    it = uncapped_iters(n, C)
    if C > 64 and it > MAXRPW:
        it = MAXRPW
    chunks = -(-C // 64) if lprl == 6 else 1
    return lprl, chunks, it, -(-nbi // it), it * G


# (n, C, lprl, chunks, iters, blocks, why): the smallest n with iters = 2 of every template, and two cases of chunked chains
MULTI_ITER = [
    (524289, 1, 0, 1, 2, 1025, "LPRL 0"),
    (262145, 2, 1, 1, 2, 1025, "LPRL 1"),
    (131073, 3, 2, 1, 2, 1025, "LPRL 2, one dead lane per row"),
    (65537, 8, 3, 1, 2, 1025, "LPRL 3"),
    (32769, 9, 4, 1, 2, 1025, "LPRL 4, 7 of 16 lanes dead"),
    (32769, 16, 4, 1, 2, 1025, "LPRL 4, no dead lane"),
    (16385, 17, 5, 1, 2, 1025, "LPRL 5, 15 of 32 lanes dead"),
    (8193, 33, 6, 1, 2, 1025, "LPRL 6, 31 of 64 lanes dead"),
    (8193, 64, 6, 1, 2, 1025, "LPRL 6, one chunk: parking off"),
    (8193, 65, 6, 2, 2, 1025, "LPRL 6, two chunks: the parked slot at it = 1"),
    (9000, 129, 6, 3, 2, 1125, "LPRL 6, three chunks: a slot parked by chunk 0, merged and parked again by chunk 1"),
    (16500, 128, 6, 2, 3, 1375, "LPRL 6, two full chunks, iters 3"),
]
TABLE = [(n, C) for n, C, *_ in MULTI_ITER]
RANKED = [(8193, 65), (65537, 8), (524289, 1), (9000, 129)]  # cond_mean with k = 3 as well as k = 0
CAP_CASE = (2097153, 65)  # iters 256 (257 without the cap), 2049 blocks, 256 rows per wavefront, one live row in the last one
NEGATIVE = [(8193, 65), (65537, 8)]
TWICE = [(9000, 129), (32769, 9)]
ALL_CHAINS = sorted(R.CHAINS + R.MORE_CHAINS)

LENGTHS = np.array([3, 8, 1, 12, 9, 0, 17, 7, 2, 16, 15, 4, 8, 20, 5, 0, 6, 9, 8, 1, 24, 3, 0, 13, 7, 10, 16, 2, 11, 8, 4, 19])
MAXLEN = int(LENGTHS.max())
INT_VALUES = np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0])
BACKWARD_EVERY, BACKWARD_AT = 11, 4


def row_lengths(n: int):
    return LENGTHS[np.arange(n) % len(LENGTHS)]


def shifts(n: int):
    """the column offset of the j-th off-diagonal entry of every row: +1, -(1 + s), +(1 + 2 s), ... below n / 2 in size, so that
    the MAXLEN columns of a row are distinct modulo n and none is the row itself"""
    assert n >= 64
    step = ((n - 1) // 2 - 2) // MAXLEN
    d = 1 + step * np.arange(MAXLEN, dtype=np.int64)
    assert step >= 1 and d[-1] < (n - 1) // 2
    return np.where(np.arange(MAXLEN) % 2 == 0, d, -d)


def int_value_index(i, j):
    """index into INT_VALUES of the off-diagonal entry j of row i (numpy arrays or torch tensors of integers)"""
    return (5 * i + 3 * j + i // 32) % 6


def backward_rows(n: int):
    return np.arange(n) % BACKWARD_EVERY == BACKWARD_AT


def build(n: int, seed: int = 0, integer: bool = False) -> R.Matrix:
    """the matrix of the module docstring as an rbstats_cases.Matrix (CSR with the diagonal stored)"""
    rng = np.random.default_rng(seed)
    rows = np.arange(n, dtype=np.int64)
    lens = row_lengths(n).astype(np.int64)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens + 1, out=rowptr[1:])
    nnz = int(rowptr[-1])
    assert nnz < 2**31
    rowid = np.repeat(rows, lens + 1)
    pos = np.arange(nnz, dtype=np.int64) - rowptr[rowid]
    back = backward_rows(n)
    dpos = np.where(back, lens, np.minimum(lens, rows % 3))[rowid]
    isdiag = pos == dpos
    j = pos - (pos > dpos)
    jj = np.minimum(j, MAXLEN - 1)  # the diagonal of a row of MAXLEN entries stored last has j = MAXLEN: unused
    col = np.where(isdiag, rowid, (rowid + shifts(n)[jj]) % n)
    if integer:
        val = INT_VALUES[int_value_index(rowid, jj)]
    else:
        val = rng.uniform(0.25, 1.0, nnz) * rng.choice([-1.0, 1.0], nnz)  # no tiny entry: the negative controls change one
    val[isdiag] = 0.0
    dom = np.bincount(rowid, weights=np.abs(val), minlength=n) + 1.0
    diag = 2.0 ** np.ceil(np.log2(dom)) if integer else dom + rng.uniform(0.0, 1.0, n)
    val[isdiag] = diag
    sel = np.nonzero(back[rowid] & ~isdiag)[0]  # contiguous per row: the diagonal of these rows is last
    order = np.lexsort((-col[sel], rowid[sel]))
    col[sel], val[sel] = col[sel][order], val[sel][order]
    name = f"geo{n}" + ("i" if integer else "")
    return R.Matrix(name, rowptr.astype(np.int32), col.astype(np.int32), val, n, f"{n} rows of 0 .. {MAXLEN} off-diagonal entries at fixed column offsets")


# ---- the reference of rbstats_cases.cond_mean_ref without a loop over rows ----------------------------------------------------------
def off_diagonal(M, rows=None):
    """(rows, ptr, cols, vals, diag): the off-diagonal entries of the given rows (all by default) in stored order, as a CSR over
    those rows, and the rows' diagonal entries"""
    rows = np.arange(M.n, dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    beg, cnt = M.rowptr[rows].astype(np.int64), (M.rowptr[rows + 1] - M.rowptr[rows]).astype(np.int64)
    local = np.repeat(np.arange(len(rows), dtype=np.int64), cnt)
    start = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(cnt, out=start[1:])
    idx = beg[local] + (np.arange(int(start[-1]), dtype=np.int64) - start[local])
    col, val = M.colidx[idx].astype(np.int64), M.vals[idx]
    isdiag = col == rows[local]
    assert np.array_equal(np.bincount(local[isdiag], minlength=len(rows)), np.ones(len(rows), np.int64))  # one stored diagonal per row
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(np.bincount(local[~isdiag], minlength=len(rows)), out=ptr[1:])
    return rows, ptr, col[~isdiag], val[~isdiag], val[isdiag]


def cond_precision_fast(M, lr=None):
    """rbstats_cases.cond_precision_host: the same float64 operations in the same order"""
    q = off_diagonal(M)[4].copy()
    if lr is not None:
        B, S = lr
        for k in range(len(S)):
            q = q + S[k] * (B[:, k] * B[:, k])
    return q


def cond_mean_ref_fast(M, Y, b=None, lr=None, rows=None, take=None):
    """(m, bound) of rbstats_cases.cond_mean_ref: np.longdouble over the j-th stored off-diagonal entry of all rows at once, every
    row's sum in its stored order (so m has the bits of the loop), the same bound_m.
    rows: only these rows (without a low-rank term); take(cols) then returns the float64 samples of the given rows of Y, which may
    live elsewhere (Y is not read), and b holds the entries of `rows` only."""
    rows_, ptr, col, val, diag = off_diagonal(M, rows)
    if take is None:
        take = lambda c: Y[c]  # noqa: E731
    C = take(rows_[:1]).shape[1]
    nr = len(rows_)
    bl = np.zeros(nr, np.longdouble) if b is None else b.astype(np.longdouble)
    length = ptr[1:] - ptr[:-1]
    s = np.zeros((nr, C), np.longdouble)
    sabs = np.zeros((nr, C), np.longdouble)
    for j in range(int(length.max()) if nr else 0):
        r = np.nonzero(length > j)[0]
        e = ptr[r] + j
        a = val[e].astype(np.longdouble)[:, None]
        y = take(col[e]).astype(np.longdouble)
        s[r] += a * y
        sabs[r] += np.abs(a) * np.abs(y)
    k = 0 if lr is None else len(lr[1])
    w = np.zeros((nr, C), np.longdouble)
    L = np.zeros((nr, C), np.longdouble)
    T = np.zeros((nr, C), np.longdouble)
    if lr is None:
        q = diag.astype(np.longdouble)
    else:
        assert rows is None
        n = M.n
        q = cond_precision_fast(M, lr).astype(np.longdouble)
        Yl = Y.astype(np.longdouble)
        Bl, Sl = lr[0].astype(np.longdouble), lr[1].astype(np.longdouble)
        t = Bl.T @ Yl  # k x C
        tabs = np.abs(Bl).T @ np.abs(Yl)
        for kk in range(k):
            bs = (Bl[:, kk] * Sl[kk])[:, None]
            by = Bl[:, kk][:, None] * Yl
            w += bs * (t[kk][None, :] - by)
            L += np.abs(bs) * (np.abs(t[kk])[None, :] + np.abs(by))
            T += np.abs(bs) * (R.gamma(n) * tabs[kk])[None, :]
    m = ((bl[:, None] - s) - w) / q[:, None]
    p = length + k + 2
    g_main = R.gamma(p.astype(np.float64)).astype(np.longdouble)[:, None]  # gamma in float64, as the loop forms it
    g_lr = R.gamma(np.maximum(p, k + 5).astype(np.float64)).astype(np.longdouble)[:, None]
    bound = (g_main * (np.abs(bl)[:, None] + sabs) + g_lr * L + T) / q[:, None]
    return m, bound


def worst_ratio(err, bound):
    """the largest err / bound; an error where the bound is zero counts as infinite"""
    safe = np.where(bound > 0, bound, 1)
    return float(np.max(np.where(bound > 0, err / safe, np.where(err > 0, np.inf, 0.0))))


# ---- the negative controls -----------------------------------------------------------------------------------------------------------
def control_row(n: int, C: int):
    """a row at it = 1 of a wavefront well inside the matrix with at least 9 off-diagonal entries"""
    lprl, _, iters, _, rpw = geometry(n, C)
    G = 64 >> lprl
    lens = row_lengths(n)
    assert iters >= 2
    for w in range(21, 21 + 64):  # from wavefront 1 of block 5 on
        for g in range(G):
            r = w * rpw + G + g
            if lens[r] >= 9:
                assert (r % rpw) // G == 1 and r < n - rpw
                return r
    raise AssertionError("no long row at it = 1")


def rows_gathering(M, column: int):
    """the rows that store `column` off their diagonal"""
    rowid = np.repeat(np.arange(M.n, dtype=np.int64), np.diff(M.rowptr.astype(np.int64)))
    return np.unique(rowid[(M.colidx == column) & (rowid != column)])


Controls = namedtuple("Controls", "M b q steps r column chain steps_y rows_y M_a")
STEPS = 3  # updates of the field tests


def controls(n: int, C: int) -> Controls:
    """the inputs of the negative controls: the matrix, right-hand side and STEPS steps of a case, and two changes at the row r
    of control_row, each 1000 in size so that the conditional means that read it move by far more than 100 bounds:
      steps_y: one sample of the last step changed, in the column of r's first stored off-diagonal entry and in a chain of chunk
               1 where the chains are chunked; rows_y are the rows that gather this column;
      M_a:     the value of that entry of r changed"""
    M = build(n, seed=n + C)
    b = R.rhs(n, seed=C)
    steps = [R.samples(n, C, seed=7 * C + s) for s in range(STEPS)]
    r = control_row(n, C)
    e = int(M.rowptr[r]) + (1 if M.colidx[M.rowptr[r]] == r else 0)  # r's first stored off-diagonal entry
    column = int(M.colidx[e])
    assert column != r
    chain = 64 if C > 64 else 5
    steps_y = [Y.copy() for Y in steps]
    steps_y[-1][column, chain] += 1000.0
    vals = M.vals.copy()
    vals[e] += 1000.0
    return Controls(M, b, cond_precision_fast(M), steps, r, column, chain, steps_y, rows_gathering(M, column), M._replace(vals=vals))
