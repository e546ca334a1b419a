"""tests/chainstats_cases.py without a GPU: geometry() is the library's pmgk_chainstats_geometry, the restated constants are the
kernels', the case table reaches what it says, the vectorised emulation has the bits of a lane-by-lane walk through
chainstats_update_kernel and chainstats_reduce_kernel, and it stays within the extended-precision bounds of
check_against_longdouble (tests/test_gpu_chainstats.py) on every small case."""
import ctypes as C_
import re
from pathlib import Path

import numpy as np
import pytest

import chainstats_cases as K
from test_gpu_chainstats import check_against_longdouble, make_qois, make_steps

SRC = (Path(__file__).resolve().parent.parent / "parmgmc_amd" / "csrc" / "kernels_chainstats.hip").read_text()
TABLE = sorted({(c.n, c.C) for c in K.CASES})
GEO = {nc: K.geometry(*nc) for nc in TABLE}


def library_geometry(n, C):
    from parmgmc_amd.capi import lib

    fn = lib.pmgk_chainstats_geometry
    fn.restype, fn.argtypes = None, [C_.c_int64, C_.c_int32, C_.POINTER(C_.c_int32), C_.POINTER(C_.c_int32)]
    it, nb = C_.c_int32(), C_.c_int32()
    fn(n, C, C_.byref(it), C_.byref(nb))
    return it.value, nb.value


def test_geometry_is_the_librarys():
    for n, C in TABLE:
        assert K.geometry(n, C)[2:4] == library_geometry(n, C), (n, C)
    # around every threshold of every chain count: one block, MAXBLK blocks | iters 2, the cap
    for C in K.COUNTS + [1000]:
        rbi = K.WAVES * (64 >> K.lpr_log2_of(C)) * K.RW
        for nbi in (1, 2, 64, 65, K.MAXBLK, K.MAXBLK + 1, 2 * K.MAXBLK + 1, K.ITER_CAP * K.MAXBLK, K.ITER_CAP * K.MAXBLK + 1, 40 * K.MAXBLK + 7):
            for n in (nbi * rbi - 1, nbi * rbi, nbi * rbi + 1):
                lprl, chunks, it, nb, rpw = K.geometry(n, C)
                assert (it, nb) == library_geometry(n, C), (n, C)
                assert rpw == it * (64 >> lprl) * K.RW and K.WAVES * nb * rpw >= n > K.WAVES * (nb - 1) * rpw  # the blocks cover the rows, none is empty
                assert chunks == 1 or rpw <= K.MAXRPW  # the parked rows fit their LDS array


def test_restated_constants_are_the_kernels():
    for name, val in (("RW", K.RW), ("MAXRPW", K.MAXRPW), ("MAXBLK", K.MAXBLK)):
        assert int(re.search(rf"constexpr int {name}\s*=\s*(\d+);", SRC).group(1)) == val, name
    assert "while (l < 6 && (1 << l) < C) ++l;" in SRC
    assert "const int64_t rbi  = 4 * (int64_t)(64 >> lprl) * RW;" in SRC and "__launch_bounds__(256)" in SRC
    assert "if (nchains > 64 && it > MAXRPW / RW) it = MAXRPW / RW;" in SRC
    assert "const int     chunks = LPRL == 6 ? (C + 63) / 64 : 1;" in SRC
    assert f"for (int b = l; b < nb; b += {K.REDUCE_SLOTS})" in SRC and "__shared__ double red[64][4];" in SRC
    for l in range(6):
        assert f"case {l}: launch_update<{l}>" in SRC
    assert "default: launch_update<6>" in SRC


def test_case_table_reaches_what_it_says():
    assert sorted(K.COUNTS) == [1, 2, 3, 4, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129]
    assert set(K.EXACT) == {(n, C) for n in (1, 63, 64, 65, 81, 1024) for C in K.COUNTS} | {(2048, 65), (2049, 65)}
    of = lambda i: {g[i] for g in GEO.values()}  # noqa: E731
    assert of(0) == set(range(7))
    # LPRL = 6 with one chunk (its chunks > 1 branch off) and with several, the chunk edges 64 | 65 and 128 | 129
    assert {(g[0], g[1]) for g in GEO.values()} >= {(6, 1), (6, 2), (6, 3)}
    assert {GEO[(1024, C)][1] for C in (33, 63, 64)} == {1} and [GEO[(1024, C)][1] for C in (65, 128, 129)] == [2, 2, 3]
    # iters >= 2 for every template, with several chunks, and 3
    multi = {(n, C): K.geometry(n, C) for n, C, _ in K.MULTI_ITER}
    assert {g[0] for g in multi.values() if g[2] >= 2} == set(range(7)) and all(g[2] >= 2 for g in multi.values())
    assert any(g[1] == 1 and g[0] == 6 for g in multi.values()) and any(g[1] == 2 for g in multi.values()) and any(g[1] == 3 for g in multi.values())
    assert multi[(70001, 128)][1:3] == (2, 3) and multi[(40000, 129)][1:3] == (3, 2)
    for (n, C), g in multi.items():  # the smallest n with iters = 2 of its template
        if (n, C) not in ((40000, 129), (70001, 128)):
            assert g[2] == 2 and K.geometry(n - 1, C)[2] == 1, (n, C)
        assert n * C * 8 <= 72e6, (n, C)
    # the cap
    assert K.geometry(*K.CAP_CASE) == (6, 2, 32, 1057, 256) and K.uncapped_iters(*K.CAP_CASE) == 34 > K.ITER_CAP
    assert K.geometry(K.CAP_CASE[0], 64)[2] == 34  # one chunk parks nothing and is not capped
    # block counts: one, and the 64 | 65 of the reduce kernel's stride; more than 1024
    assert {1, 64, 65} <= of(3) and GEO[(2048, 65)][3] == 64 and GEO[(2049, 65)][3] == 65 and max(of(3)) > K.MAXBLK
    # a last block with idle wavefronts, a last wavefront with a cut row group, and neither
    assert any(K.idle_wavefronts(n, C) == 3 for n, C in K.EXACT) and any(K.idle_wavefronts(n, C) == 0 for n, C in K.EXACT)
    for lprl in range(6):
        assert any(K.partial_row_group(n, C) and GEO[(n, C)][0] == lprl for n, C in TABLE), lprl
    assert any(not K.partial_row_group(n, C) and GEO[(n, C)][0] == 0 for n, C in K.EXACT)
    assert any(K.idle_wavefronts(n, C) > 0 and g[2] >= 2 for (n, C), g in multi.items())
    # the negative controls: a one-block-per-32-rows chunked case with iters 1, a chunked one with iters 2, LPRL 4 with iters 2
    assert [K.geometry(n, C)[:3] for n, C in K.NEGATIVE] == [(6, 3, 1), (6, 2, 2), (4, 1, 2)]
    assert [K.geometry(n, C)[:3] for n, C in K.TWICE] == [(6, 3, 2), (4, 1, 2)]


# ---- a lane-by-lane walk through the kernels' code (not through the header's prose) ----------------------------------------------
def kernel_walk(Y, qois, N, mean, M2, iters, nb):
    """one pmgk_chainstats_update: returns (mean, M2, trace_step[q][c]); arrays of 64 stand for a wavefront's lanes"""
    n, C = Y.shape
    nq = len(qois)
    lprl = K.lpr_log2_of(C)
    LPR, G = 1 << lprl, 64 >> lprl
    RWI = G * K.RW
    lane = np.arange(64)
    g, cl = lane >> lprl, lane & (LPR - 1)
    chunks = -(-C // 64) if lprl == 6 else 1
    mean, M2 = mean.copy(), M2.copy()
    partial = np.zeros((nb, nq, C))
    shfl = lambda v, o: v[lane ^ o]  # noqa: E731
    for B in range(nb):
        parked = {}
        for k in range(chunks):
            red = np.zeros((4, nq, 64))
            c = k * 64 + cl
            live = c < C
            cc = np.minimum(c, C - 1)
            cnt, seen, last = float(min(64, C - k * 64)), 64.0 * k, k == chunks - 1
            for wv in range(4):
                row0 = (B * 4 + wv) * iters * RWI
                acc = np.zeros((nq, 64))
                for it in range(iters):
                    rb = row0 + it * RWI + g
                    rows = [rb + i * G for i in range(K.RW)]
                    y = [np.where(live & (r < n), Y[np.minimum(r, n - 1), cc], 0.0) for r in rows]
                    for q, w in enumerate(qois):
                        for i in range(K.RW):
                            acc[q] = acc[q] + (y[i] if w is None else np.where(rows[i] < n, w[np.minimum(rows[i], n - 1)], 0.0) * y[i])
                    for i in range(K.RW):
                        s = y[i]
                        o = 1
                        while o < LPR:
                            s = s + shfl(s, o)
                            o <<= 1
                        cm = s / cnt
                        d = np.where(live, y[i] - cm, 0.0)
                        t = d * d
                        o = 1
                        while o < LPR:
                            t = t + shfl(t, o)
                            o <<= 1
                        bm, bM2 = cm, t
                        if lprl == 6 and chunks > 1:
                            slot = (wv * K.MAXRPW + it * K.RW + i) * 2
                            if k > 0:
                                bm, bM2 = K._merge(seen, np.full(64, parked[slot]), np.full(64, parked[slot + 1]), cnt, cm, t)
                            if not last:
                                parked[slot], parked[slot + 1] = bm[0], bM2[0]
                        if last:
                            for l in np.nonzero((cl == 0) & (rows[i] < n))[0]:
                                r = rows[i][l]
                                mean[r], M2[r] = K._merge(N, mean[r], M2[r], float(C), bm[l], bM2[l])
                for q in range(nq):
                    v = acc[q]
                    o = LPR
                    while o < 64:
                        v = v + shfl(v, o)
                        o <<= 1
                    red[wv, q, cl[g == 0]] = v[g == 0]
            for q in range(nq):
                for x in range(LPR):
                    if k * 64 + x < C:
                        partial[B, q, k * 64 + x] = (red[0, q, x] + red[1, q, x]) + (red[2, q, x] + red[3, q, x])
    out = np.zeros((nq, C))
    for q in range(nq):
        a = np.zeros((64, C))
        for l in range(64):
            for b in range(l, nb, 64):
                a[l] = a[l] + partial[b, q]
        o = 32
        while o >= 1:
            a[:o] = a[:o] + a[o : 2 * o]
            o >>= 1
        out[q] = a[0]
    return mean, M2, out


@pytest.mark.parametrize("n,C,iters", [(1, 1, 1), (81, 1, 1), (65, 2, 1), (81, 3, 1), (300, 9, 2), (81, 16, 1), (130, 17, 3), (65, 64, 2), (97, 65, 2), (70, 129, 3), (2049, 65, 1)])
def test_emulation_has_the_bits_of_a_walk_through_the_kernels(n, C, iters, monkeypatch):
    """iters > 1 at sizes a Python loop can walk: the geometry is handed to both with the block count that iters leaves"""
    lprl, chunks, it0, nb0, _ = K.geometry(n, C)
    rbi = K.WAVES * (64 >> lprl) * K.RW
    nb = -(-(-(-n // rbi)) // iters)
    assert it0 == 1 and (iters > 1 or nb == nb0)
    monkeypatch.setattr(K, "geometry", lambda n_, C_: (lprl, chunks, iters, nb, iters * (64 >> lprl) * K.RW))
    steps = make_steps(n, C, 3, 50.0, seed=n + C)
    qois = make_qois(n, 3, seed=C)
    em = K.emulate(steps, qois)
    mean, M2 = np.zeros(n), np.zeros(n)
    for t, Y in enumerate(steps):
        mean, M2, tr = kernel_walk(Y, qois, float(t * C), mean, M2, iters, nb)
        for q in range(3):
            assert np.array_equal(tr[q], em.trace(q)[t]), (t, q)
    m_em, v_em = em.fields_host()
    assert np.array_equal(mean, m_em) and np.array_equal(M2 / (3.0 * C - 1.0), v_em)


def test_emulation_depends_on_the_order():
    """the bits are the order's: numpy's own sums of the same numbers differ from them somewhere"""
    steps = make_steps(1024, 129, 3, 50.0, seed=1)
    em = K.emulate(steps, [None])
    allY = np.concatenate(steps, axis=1)
    assert not np.array_equal(em.fields_host()[0], allY.mean(axis=1))
    assert not np.array_equal(em.trace(0), np.array([Y.sum(axis=0) for Y in steps]))


@pytest.mark.parametrize("n,C", K.EXACT)
def test_emulation_within_the_longdouble_bounds(n, C):
    for offset in (0.0, 50.0):
        steps = make_steps(n, C, 3, offset, seed=n + 7 * C + 3)
        qois = make_qois(n, 4, seed=C)
        check_against_longdouble(K.emulate(steps, qois), steps, qois, f"emulation n={n} C={C} offset={offset}")
