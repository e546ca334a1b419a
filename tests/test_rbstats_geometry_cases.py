"""tests/rbstats_geometry_cases.py without a GPU: geometry() is the library's pmgk_rbstats_geometry, the restated constants are
the kernel's, the case table reaches what it says, the built matrices hold the rows they are there for, the vectorised reference
has the bits of the loop of rbstats_cases.cond_mean_ref (m np.array_equal in np.longdouble: every row's sum runs in its stored
order in both; the bounds are equal too), the integer variant's results are float64 numbers, and the negative controls of
tests/test_gpu_rbstats_geometry.py move their rows by at least 100 bounds."""
import ctypes as C_
import re
from pathlib import Path

import numpy as np
import pytest

import rbstats_cases as R
import rbstats_geometry_cases as K

SRC = (Path(__file__).resolve().parent.parent / "parmgmc_amd" / "csrc" / "kernels_rbstats.hip").read_text()


def library_geometry(n, C):
    from parmgmc_amd.capi import lib

    fn = lib.pmgk_rbstats_geometry
    fn.restype, fn.argtypes = None, [C_.c_int64, C_.c_int32, C_.POINTER(C_.c_int32), C_.POINTER(C_.c_int32)]
    it, nb = C_.c_int32(), C_.c_int32()
    fn(n, C, C_.byref(it), C_.byref(nb))
    return it.value, nb.value


def check_geometry(n, C):
    lprl, chunks, it, nb, rpw = K.geometry(n, C)
    assert (it, nb) == library_geometry(n, C), (n, C)
    assert rpw == it * (64 >> lprl) and K.WAVES * nb * rpw >= n > K.WAVES * (nb - 1) * rpw, (n, C)  # the blocks cover the rows, none is empty
    assert chunks == 1 or it <= K.MAXRPW, (n, C)  # the parked rows fit their LDS array
    assert chunks == (1 if C <= 64 else -(-C // 64))


def test_geometry_is_the_librarys():
    for n, C, lprl, chunks, iters, nb, _ in K.MULTI_ITER:
        assert K.geometry(n, C) == (lprl, chunks, iters, nb, iters * (64 >> lprl)), (n, C)
        check_geometry(n, C)
    for n, C in [K.CAP_CASE, (K.CAP_CASE[0], 64)]:
        check_geometry(n, C)
    # around every threshold of every chain count: one block, MAXBLK blocks | iters 2, the cap
    for C in K.ALL_CHAINS + [1000]:
        rbi = K.WAVES * (64 >> K.lpr_log2_of(C))
        for nbi in (1, 2, K.MAXBLK, K.MAXBLK + 1, 2 * K.MAXBLK + 1, K.MAXRPW * K.MAXBLK, K.MAXRPW * K.MAXBLK + 1):
            for n in (nbi * rbi - 1, nbi * rbi, nbi * rbi + 1):
                check_geometry(n, C)


def test_restated_constants_are_the_kernels():
    for name, val in (("BATCH", K.BATCH), ("MAXRPW", K.MAXRPW), ("MAXBLK", K.MAXBLK)):
        assert int(re.search(rf"constexpr int {name}\s*=\s*(\d+);", SRC).group(1)) == val, name
    assert "while (l < 6 && (1 << l) < C) ++l;" in SRC
    assert "const int64_t rbi = 4 * (int64_t)(64 >> lpr_log2_of(nchains));" in SRC and "__launch_bounds__(256)" in SRC
    assert "if (nchains > 64 && it > MAXRPW) it = MAXRPW;" in SRC  # the cap
    assert "__shared__ double parked[LPRL == 6 && !STORE ? 4 * MAXRPW * 2 : 2];" in SRC
    assert "chunk_batch(parked + (wv * MAXRPW + it) * 2, k, last, lane, seen, cnt, cm, cM2, bm, bM2);" in SRC
    assert "const int64_t row = row0 + (int64_t)it * G + g;" in SRC
    assert "const int     chunks = LPRL == 6 ? (C + 63) / 64 : 1;" in SRC
    for l in range(6):
        assert f"case {l}: launch<{l}>" in SRC
    assert "default: launch<6>" in SRC


def test_case_table_reaches_what_it_says():
    assert K.ALL_CHAINS == [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 130]
    geo = {(n, C): K.geometry(n, C) for n, C in K.TABLE}
    assert {g[0] for g in geo.values() if g[2] == 2} == set(range(7))  # every template at iters 2
    assert all(g[2] >= 2 and g[3] <= K.MAXBLK for g in geo.values())
    assert any(g[1] == 2 and g[2] >= 2 for g in geo.values()) and any(g[1] == 3 and g[2] >= 2 for g in geo.values())
    assert geo[(8193, 64)][:3] == (6, 1, 2) and geo[(8193, 65)][:3] == (6, 2, 2) and geo[(9000, 129)][:3] == (6, 3, 2) and geo[(16500, 128)][:3] == (6, 2, 3)
    for (n, C), g in geo.items():
        if (n, C) not in ((9000, 129), (16500, 128)):  # the smallest n with iters = 2 of its template
            assert g[2] == 2 and K.geometry(n - 1, C)[2] == 1, (n, C)
        assert n * C * 8 < 20e6, (n, C)
    assert set(K.RANKED) <= set(K.TABLE) and set(K.NEGATIVE) <= set(K.TABLE) and set(K.TWICE) <= set(K.TABLE)
    assert [geo[nc][:3] for nc in K.NEGATIVE] == [(6, 2, 2), (3, 1, 2)]
    assert [geo[nc][:3] for nc in K.TWICE] == [(6, 3, 2), (4, 1, 2)]
    # the cap: iters 256 where 257 are asked for, more than MAXBLK blocks, one live row in the last wavefront
    n, C = K.CAP_CASE
    assert K.geometry(n, C) == (6, 2, K.MAXRPW, 2049, 256) and K.uncapped_iters(n, C) == 257 and 2049 > K.MAXBLK
    assert (-(-n // 256) - 1) * 256 == n - 1 == 2097152
    assert K.geometry(n, 64)[1:3] == (1, 257)  # one chunk parks nothing and is not capped


@pytest.mark.parametrize("n,C", K.TABLE + [K.CAP_CASE])
def test_row_lengths_at_the_positions_of_every_case(n, C):
    lprl, _, iters, _, rpw = K.geometry(n, C)
    G = 64 >> lprl
    lens = K.row_lengths(n)
    it = (np.arange(n) % rpw) // G
    for cls in (lens == 0, (lens >= 1) & (lens <= 7), lens == 8, (lens >= 9) & (lens <= 15), lens > 16):
        if (n, C) == K.CAP_CASE:  # 256 rows per wavefront are eight periods of LENGTHS: it fixes the length
            assert cls[it >= 1].any() and lens[n - 1] > 0 and lens[it == 1].all() and lens[it == 255].all()
        else:
            assert cls[it == 1].any()  # every class, the empty and the long rows among them, at it = 1
    if G >= 2:  # every whole group of G consecutive rows served together holds rows of different length
        whole = lens[: n // G * G].reshape(-1, G)
        assert (whole.min(axis=1) < whole.max(axis=1)).all()
    sh = K.shifts(n)
    assert len(set(sh % n)) == K.MAXLEN and 0 not in set(sh % n)  # distinct columns, none the diagonal
    assert (np.abs(sh[:2]) < rpw).any() and (np.abs(sh) >= K.WAVES * rpw).any() and (sh > 0).any() and (sh < 0).any()
    if iters >= 2 and G == 1:
        assert abs(sh[0]) == 1  # the next row: another iteration of the same wavefront


@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("n", [300, 8193, 32769])
def test_built_matrix_holds_its_rows(n, integer):
    M = K.build(n, seed=n, integer=integer)
    assert M.n == n and M.rowptr[0] == 0 and M.rowptr[-1] == len(M.colidx) == len(M.vals) and M.colidx.dtype == np.int32
    lens = K.row_lengths(n)
    assert np.array_equal(np.diff(M.rowptr), lens + 1)
    sh, back = K.shifts(n), K.backward_rows(n)
    for i in list(range(70)) + list(range(n - 40, n)):  # the stored layout, row by row, at both ends
        cols = M.colidx[M.rowptr[i] : M.rowptr[i + 1]].astype(np.int64)
        vals = M.vals[M.rowptr[i] : M.rowptr[i + 1]]
        want = [(i + int(s)) % n for s in sh[: lens[i]]]
        assert sorted(cols) == sorted(want + [i]) and len(set(cols)) == lens[i] + 1
        if back[i]:
            assert cols[-1] == i and list(cols[:-1]) == sorted(want, reverse=True)
        else:
            d = min(lens[i], i % 3)
            assert cols[d] == i and list(np.delete(cols, d)) == want
        off = np.abs(vals[cols != i])
        diag = vals[cols == i][0]
        assert diag >= off.sum() + 1 and np.isfinite(vals).all()
        if integer:
            assert set(off) <= {1.0, 2.0, 3.0} and np.log2(diag) == np.round(np.log2(diag))
            if not back[i]:
                assert list(vals[cols != i]) == [K.INT_VALUES[K.int_value_index(i, j)] for j in range(lens[i])]
        else:
            assert (off >= 0.25).all() and (off <= 1.0).all()
    assert any(back[i] and lens[i] > 2 for i in range(70))  # a row stored backwards has an order to speak of
    rows, ptr, col, val, diag = K.off_diagonal(M)
    assert np.array_equal(ptr[1:] - ptr[:-1], lens) and (col != np.repeat(rows, lens)).all() and (diag > 0).all()
    assert np.array_equal(K.cond_precision_fast(M), diag)


def _cases_of_the_reference():
    return [R.random_spd(65, 65), R.random_spd(257, 257), K.build(300, seed=3)]


@pytest.mark.parametrize("M", _cases_of_the_reference(), ids=lambda M: M.name)
@pytest.mark.parametrize("k", [0, 3])
def test_fast_reference_has_the_bits_of_the_loop(M, k):
    C = 5
    Y = R.samples(M.n, C, seed=M.n + k)
    lr = R.lowrank(M.n, k, seed=M.n)
    assert np.array_equal(K.cond_precision_fast(M, lr), R.cond_precision_host(M, lr))
    for b in (R.rhs(M.n, seed=k), None):
        m, bound = R.cond_mean_ref(M, Y, b, lr)
        mf, boundf = K.cond_mean_ref_fast(M, Y, b, lr)
        assert mf.dtype == np.longdouble and np.array_equal(mf, m)
        assert (boundf >= bound).all() and np.array_equal(boundf, bound)
        if k == 0:  # some rows only, the samples fetched through take()
            rows = np.array([0, 3, 7, 11, M.n - 1, 40, 40])
            ms, bs = K.cond_mean_ref_fast(M, None, None if b is None else b[rows], rows=rows, take=lambda c: Y[c])
            assert np.array_equal(ms, m[rows]) and np.array_equal(bs, bound[rows])


@pytest.mark.parametrize("n,C", [(300, 5), (8193, 65), (32769, 9)])
def test_integer_variant_is_exact_in_float64(n, C):
    M = K.build(n, integer=True)
    Y = R.samples(n, C, seed=C, integer=True)
    b = R.rhs(n, seed=C, integer=True)
    m, bound = K.cond_mean_ref_fast(M, Y, b)
    assert np.array_equal(m.astype(np.float64).astype(np.longdouble), m)
    # restated with shifted copies of Y, the way the cap test restates it on the device: float64 throughout, nothing rounds
    lens, sh = K.row_lengths(n), K.shifts(n)
    i = np.arange(n)
    s = np.zeros((n, C))
    for j in range(K.MAXLEN):
        a = K.INT_VALUES[K.int_value_index(i, j)]
        s += np.where((lens > j)[:, None], a[:, None] * np.roll(Y, -int(sh[j]), axis=0), 0.0)
    assert np.array_equal((b[:, None] - s) / K.cond_precision_fast(M)[:, None], m.astype(np.float64))


@pytest.mark.parametrize("n,C", K.NEGATIVE)
def test_negative_controls_move_the_reference(n, C):
    """the two changes of test_gpu_rbstats_geometry.test_one_change_is_seen_where_it_belongs, on the references alone"""
    ctl = K.controls(n, C)
    assert (ctl.r % K.geometry(n, C)[4]) // (64 >> K.geometry(n, C)[0]) == 1
    assert ctl.r in ctl.rows_y and ctl.chain // 64 == min(1, K.geometry(n, C)[1] - 1)
    m0 = [K.cond_mean_ref_fast(ctl.M, Y, ctl.b) for Y in ctl.steps]
    f0 = R.fields_reference([m for m, _ in m0], [bd for _, bd in m0], ctl.q)
    for what, (M1, steps1, rows, chains) in (("y", (ctl.M, ctl.steps_y, ctl.rows_y, [ctl.chain])), ("a", (ctl.M_a, ctl.steps, np.array([ctl.r]), list(range(C))))):
        m1 = [K.cond_mean_ref_fast(M1, Y, ctl.b) for Y in steps1]
        f1 = R.fields_reference([m for m, _ in m1], [bd for _, bd in m1], ctl.q)
        others = np.ones(n, bool)
        others[rows] = False
        for t in range(len(ctl.steps)):
            moved = np.abs(m1[t][0] - m0[t][0])
            hit = np.zeros((n, C), bool)
            if what == "a" or t == len(ctl.steps) - 1:  # the sample is changed in the last step only
                hit[np.ix_(rows, chains)] = True
            assert (moved[hit] >= 100 * m0[t][1][hit]).all() and (moved[~hit] == 0).all(), (what, t)
        assert (np.abs(f1[0] - f0[0])[rows] >= 100 * f0[2][rows]).all() and (np.abs(f1[1] - f0[1])[rows] >= 100 * f0[3][rows]).all(), what
        assert np.array_equal(f1[0][others], f0[0][others]) and np.array_equal(f1[1][others], f0[1][others])
