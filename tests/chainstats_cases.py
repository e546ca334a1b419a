"""Launch geometry, cases and a float64 emulation of the order of every sum of the chain statistics kernels
(kernels_chainstats.hip).  Importable without a device; tests/test_chainstats_cases.py checks this module on the CPU,
tests/test_gpu_chainstats_splits.py runs the library against it.

geometry(n, C) restates lpr_log2_of and pmgk_chainstats_geometry: lpr = C rounded up to a power of two (at most 64) lanes share
a row, a wavefront serves G = 64 / lpr rows at a time, RW = 8 such groups per iteration, four wavefronts per block; more than
MAXBLK = 1024 blocks' worth of rows gives every wavefront iters > 1 iterations, and chains beyond 64 (taken in chunks of 64 by
the same wavefront) cap iters at MAXRPW / RW = 32, the rows whose (mean, M2) a wavefront can park in LDS between chunks.

CASES names what every (n, C) the GPU tests launch is there for; the chain counts are CONTROLS + CHAINS of
tests/woodbury_cases.py.

Emulation follows the kernel header's ORDER OF EVERY SUM, one IEEE float64 operation per numpy operation (numpy neither fuses
nor reorders elementwise arithmetic; no np.sum anywhere): the device results are expected to have exactly its bits.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from woodbury_cases import CHAINS, CONTROLS

RW = 8  # row groups a wavefront keeps in flight
MAXRPW = 256  # rows per wavefront when the chains are chunked
MAXBLK = 1024  # blocks of the update before iters grows
WAVES = 4  # wavefronts per block
REDUCE_SLOTS = 64  # chainstats_reduce_kernel: slot l adds the blocks l, l + 64, ...
ITER_CAP = MAXRPW // RW

COUNTS = CONTROLS + CHAINS


def lpr_log2_of(C: int) -> int:
    l = 0
    while l < 6 and (1 << l) < C:
        l += 1
    return l


def uncapped_iters(n: int, C: int) -> int:
    rbi = WAVES * (64 >> lpr_log2_of(C)) * RW  # rows of a block per iteration
    nbi = -(-n // rbi)
    return max(1, -(-nbi // MAXBLK))


def geometry(n: int, C: int):
    """(lprl, chunks, iters, nblocks, rows_per_wavefront) of one update of an n x C step"""
    lprl = lpr_log2_of(C)
    G = 64 >> lprl
    rbi = WAVES * G * RW
    nbi = -(-n // rbi)
    it = uncapped_iters(n, C)
    if C > 64 and it > ITER_CAP:
        it = ITER_CAP
    chunks = -(-C // 64) if lprl == 6 else 1
    return lprl, chunks, it, -(-nbi // it), it * G * RW


def idle_wavefronts(n: int, C: int) -> int:
    """wavefronts of the last block whose first row is beyond the matrix"""
    _, _, _, nb, rpw = geometry(n, C)
    return WAVES * nb - -(-n // rpw)


def partial_row_group(n: int, C: int) -> bool:
    """the last live wavefront's last group of G rows is cut by the end of the matrix"""
    return n % (64 >> lpr_log2_of(C)) != 0


Case = namedtuple("Case", "n C part why")

EXACT_NS = [1, 63, 64, 65, 81, 1024]
EXACT_WHY = {
    1: "one row: one live lane group, three idle wavefronts, one block",
    63: "one row short of a full wavefront of the C = 1 split",
    64: "64 rows: whole row groups at every split",
    65: "one row into the next row group",
    81: "odd row count of the existing suite",
    1024: "several blocks at every split; C = 1: half a block",
}
# the smallest n with iters = 2 per template; the last one has iters = 3 and no dead lane in its chunks
MULTI_ITER = [
    (2097153, 1, "LPRL 0, iters 2"),
    (1048577, 2, "LPRL 1, iters 2, no dead lane"),
    (524289, 3, "LPRL 2, iters 2, one dead lane per row"),
    (262145, 8, "LPRL 3, iters 2, no dead lane"),
    (131073, 9, "LPRL 4, iters 2, 7 of 16 lanes dead"),
    (131073, 16, "LPRL 4, iters 2, no dead lane"),
    (65537, 17, "LPRL 5, iters 2, 15 of 32 lanes dead"),
    (32769, 64, "LPRL 6, one chunk (the chunks > 1 branch off), iters 2"),
    (32769, 65, "LPRL 6, two chunks, iters 2: the parked slot at it = 1"),
    (40000, 129, "LPRL 6, three chunks, iters 2: a slot parked by chunk 0, merged and parked again by chunk 1"),
    (70001, 128, "LPRL 6, two full chunks, iters 3"),
]
CAP_CASE = (1081345, 65)  # iters 32 (34 without the cap), 1057 blocks, 256 rows per wavefront
NEGATIVE = [(1024, 129), (32769, 65), (131073, 16)]
TWICE = [(40000, 129), (131073, 9)]

CASES = (
    [Case(n, C, "exact", EXACT_WHY[n]) for n in EXACT_NS for C in COUNTS]
    + [Case(2048, 65, "exact", "64 blocks: every slot of the reduce kernel adds one block"), Case(2049, 65, "exact", "65 blocks: slot 0 of the reduce kernel adds a second block")]
    + [Case(n, C, "iters", why) for n, C, why in MULTI_ITER]
    + [Case(*CAP_CASE, "cap", "chunked chains above 32 * 32 * 1024 rows: iters capped at 32, more than 1024 blocks")]
    + [Case(n, C, "negative", "one changed entry is seen where it belongs and nowhere else") for n, C in NEGATIVE]
    + [Case(n, C, "twice", "the same bits on a second run on a side stream") for n, C in TWICE]
)
EXACT = [(c.n, c.C) for c in CASES if c.part == "exact"]


# ---- the sums in the kernels' order ------------------------------------------------------------------------------------------------
def _pairs_tree(v, axis):
    """balanced tree over a power-of-two axis, neighbours first (slot i with i ^ 1, then i ^ 2, ...)"""
    v = np.moveaxis(v, axis, 0)
    while v.shape[0] > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def _merge(N, m, M, Nb, mb, Mb):
    """(Nb, mb, Mb) merged into (N, m, M): merge() of the kernel, operand for operand"""
    d = mb - m
    Np = N + Nb
    return m + (d * Nb) / Np, M + (Mb + (((d * d) * N) * Nb) / Np)


def batch_of_step(Y):
    """(bm, bM2) of every row over the C chains of one step"""
    n, C = Y.shape
    lprl, chunks, *_ = geometry(n, C)
    lpr = 1 << lprl
    bm = bM2 = None
    for k in range(chunks):
        cnt = min(64, C - 64 * k)
        y = np.zeros((n, lpr))
        y[:, :cnt] = Y[:, 64 * k : 64 * k + cnt]
        cm = _pairs_tree(y, 1) / np.float64(cnt)
        d = np.zeros((n, lpr))
        d[:, :cnt] = y[:, :cnt] - cm[:, None]
        cM2 = _pairs_tree(d * d, 1)
        if k == 0:
            bm, bM2 = cm, cM2
        else:
            bm, bM2 = _merge(np.float64(64.0 * k), bm, bM2, np.float64(cnt), cm, cM2)
    return bm, bM2


def qoi_of_step(Y, w):
    """w . Y[:, c] of every chain (w = None: all ones, no multiplication) in the order of the update and reduce kernels"""
    n, C = Y.shape
    lprl, _, iters, nb, rpw = geometry(n, C)
    G = 64 >> lprl
    P = np.zeros((nb * WAVES * rpw, C))  # rows beyond n: w = 0.0 times y = 0.0
    P[:n] = Y if w is None else w[:, None] * Y
    P = P.reshape(nb * WAVES, iters * RW, G, C)  # row = wavefront * rpw + j * G + g
    acc = np.zeros((nb * WAVES, G, C))
    for j in range(iters * RW):
        acc = acc + P[:, j]
    wave = _pairs_tree(acc, 1).reshape(nb, WAVES, C)
    block = (wave[:, 0] + wave[:, 1]) + (wave[:, 2] + wave[:, 3])
    rounds = -(-nb // REDUCE_SLOTS)
    padded = np.zeros((rounds * REDUCE_SLOTS, C))  # a slot never holds -0.0 after its first addition: +0.0 changes nothing
    padded[:nb] = block
    padded = padded.reshape(rounds, REDUCE_SLOTS, C)
    slot = np.zeros((REDUCE_SLOTS, C))
    for r in range(rounds):
        slot = slot + padded[r]
    o = REDUCE_SLOTS // 2
    while o >= 1:  # t with t + 32, t + 16, ... t + 1
        slot = slot[:o] + slot[o : 2 * o]
        o //= 2
    return slot[0]


class _Host:
    """what check_against_longdouble of tests/test_gpu_chainstats.py asks of a field: .cpu().numpy()"""

    def __init__(self, a):
        self._a = a

    def cpu(self):
        return self

    def numpy(self):
        return self._a


class Emulation:
    """ChainStats restated: update(Y) per step, fields() and trace(q) as the handle gives them"""

    def __init__(self, n, C, qois):
        self.n, self.C, self.qois = n, C, list(qois)
        self.steps = 0
        self.mean, self.M2 = np.zeros(n), np.zeros(n)
        self.traces = [[] for _ in self.qois]

    def update(self, Y):
        Y = np.ascontiguousarray(Y, np.float64)
        assert Y.shape == (self.n, self.C)
        bm, bM2 = batch_of_step(Y)
        N = np.float64(self.steps) * np.float64(self.C)
        self.mean, self.M2 = _merge(N, self.mean, self.M2, np.float64(self.C), bm, bM2)
        for q, w in enumerate(self.qois):
            self.traces[q].append(qoi_of_step(Y, w))
        self.steps += 1

    def fields_host(self):
        count = np.float64(self.steps) * np.float64(self.C)
        return self.mean, self.M2 / (count - 1.0)

    def fields(self):
        return tuple(_Host(a) for a in self.fields_host())

    def trace(self, q):
        return np.array(self.traces[q]).reshape(self.steps, self.C)


def emulate(steps, qois) -> Emulation:
    n, C = steps[0].shape
    em = Emulation(n, C, qois)
    for Y in steps:
        em.update(Y)
    return em


# ---- extended-precision reference of the fields with the bounds of check_against_longdouble ---------------------------------------
EPS = np.finfo(np.float64).eps


def longdouble_fields(steps):
    """(m_ref, v_ref, mean_bound, var_bound): the reference and bounds check_against_longdouble forms, for the negative controls"""
    T, (_, C) = len(steps), steps[0].shape
    allY = np.concatenate(steps, axis=1).astype(np.longdouble)
    m_ref = allY.sum(axis=1) / (T * C)
    v_ref = ((allY - m_ref[:, None]) ** 2).sum(axis=1) / (T * C - 1)
    return m_ref, v_ref, T * C * EPS * float(np.abs(allY).max()), 16 * T * C * EPS * float((v_ref + m_ref**2).max())


def longdouble_qoi(Y, w, c):
    """(ref, bound) of QOI w on chain c of one step, as check_against_longdouble forms them"""
    n = Y.shape[0]
    g = n * EPS / (1 - n * EPS)
    wl = np.ones(n, np.longdouble) if w is None else w.astype(np.longdouble)
    yl = Y[:, c].astype(np.longdouble)
    return wl @ yl, g * (np.abs(wl) * np.abs(yl)).sum()
