"""The Rao-Blackwellised statistics kernel (rbstats_kernel, kernels_rbstats.hip) at every launch geometry of
tests/rbstats_geometry_cases.py:

  a. cond_mean with several iterations per wavefront (the row index row0 + it * G + g of every template, rows of every length
     class at it >= 1) within bound_m of the np.longdouble reference, exact on integer data, written into a buffer whose sentinels
     before the first row and after the last one stay as they were;
  b. three updates at the same sizes (the parked LDS slot of chunked chains at it >= 1): the bits of a ChainStats fed the
     conditional means, the fields within the bounds of rbstats_cases.fields_reference, the same bits after reset() on a side
     stream;
  c. the iteration cap of chunked chains (2097153 rows: iters 256 where 257 are asked for, 2049 blocks, one live row in the last
     wavefront) on integer data generated on the device: every conditional mean equals the exact one, formed with shifted copies
     of Y in plain torch; the fields have the bits of ChainStats and lie within the bounds on about 4000 rows;
  d. negative controls: one changed sample, and one changed matrix entry, of a row at it = 1 move the rows that read them out of
     the bounds taken around the unchanged reference, and no other row by a bit.
Observed on the MI355X: a. worst |m - ref| / bound over the twelve cases 0.412 (k = 0; n = 262145, C = 2), 0.105 (k = 3); the integer
results equal, every sentinel unchanged.  b. every bit equal; worst error / bound: mean 3.9e-2 (n = 262145, C = 2), variance
7.7e-3.  c. all 136 314 945 conditional means of both steps equal; fields: mean 2.0e-3, variance 1.4e-4 of the bound on 4068 rows.
d. the rows named leave their bounds by factors of 9e11 to 1e17, every other row keeps its bits."""
import functools

import numpy as np
import pytest

import rbstats_cases as R
import rbstats_geometry_cases as K
from test_gpu_rbstats import dev, host, make_rb

pytestmark = pytest.mark.gpu
IDS = [f"{n}-{C_}" for n, C_ in K.TABLE]
SENTINEL = -1.2345e300
FRONT = 1024  # sentinel doubles before the first row


@functools.lru_cache(maxsize=2)
def matrix(n, integer=False):
    return K.build(n, seed=n, integer=integer)


def cond_mean_guarded(rb, Yd):
    """pmg_rbstats_cond_mean into the middle of a larger buffer: FRONT sentinels before M and, behind it, more than the rows past
    n of the last block (4 wavefronts of iters * G rows of C entries) could fill"""
    import torch

    from parmgmc_amd.capi import check, lib
    from parmgmc_amd.wrappers import _ptr, _stream

    n, C_ = rb.n, rb.nchains
    rpw = K.geometry(n, C_)[4]
    back = K.WAVES * rpw * C_ + 64
    buf = torch.full((FRONT + n * C_ + back,), SENTINEL, dtype=torch.float64, device="cuda")
    M = buf[FRONT : FRONT + n * C_]
    check(lib.pmg_rbstats_cond_mean(rb._h, _ptr(Yd), _ptr(M), _stream()))
    assert bool((buf[:FRONT] == SENTINEL).all()), "written before the first row"
    assert bool((buf[FRONT + n * C_ :] == SENTINEL).all()), "written behind the last row"
    return M.view(n, C_)


def check_fields(mean, var, refs, q, label):
    m_ref, v_ref, mean_bound, var_bound = R.fields_reference([r[0] for r in refs], [r[1] for r in refs], q)
    mean_err, var_err = np.abs(mean - m_ref), np.abs(var - v_ref)
    print(f"{label}: mean err / bound {float((mean_err / mean_bound).max()):.3e}; var err / bound {float((var_err / var_bound).max()):.3e}")
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    assert (mean_err <= mean_bound).all(), label
    assert (var_err <= var_bound).all(), label


# ---- a. cond_mean at several iterations per wavefront ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C_", K.TABLE, ids=IDS)
def test_cond_mean_at_several_iterations(n, C_):
    lprl, chunks, iters, nb, rpw = K.geometry(n, C_)
    assert iters >= 2 and nb <= K.MAXBLK
    M = matrix(n)
    Y = R.samples(n, C_, seed=n + C_)
    b = R.rhs(n, seed=C_)
    rb = make_rb(M, C_)
    Yd = dev(Y)
    for k in (0, 3) if (n, C_) in K.RANKED else (0,):
        lr = R.lowrank(n, k, seed=n)
        rb.set_lowrank(*(lr or (None, None)))
        for rhs_ in (b, None):
            rb.set_rhs(None if rhs_ is None else dev(rhs_))
            got = host(cond_mean_guarded(rb, Yd))
            ref, bound = K.cond_mean_ref_fast(M, Y, rhs_, lr)
            err = np.abs(got.astype(np.longdouble) - ref)
            worst = K.worst_ratio(err, bound)
            print(f"n={n} C={C_} LPRL={lprl} chunks={chunks} iters={iters} k={k} b={'yes' if rhs_ is not None else 'zero'}: worst err / bound {worst:.3f}")
            assert np.isfinite(got).all()
            assert (err <= bound).all(), (n, C_, k, worst)
    assert rb.count() == (0, 0)
    # integer data: nothing rounds
    Mi = matrix(n, integer=True)
    Yi = R.samples(n, C_, seed=C_, integer=True)
    bi = R.rhs(n, seed=C_, integer=True)
    ref, _ = K.cond_mean_ref_fast(Mi, Yi, bi)
    want = ref.astype(np.float64)
    assert np.array_equal(want.astype(np.longdouble), ref)  # the exact result is a float64
    got = host(cond_mean_guarded(make_rb(Mi, C_, b=bi), dev(Yi)))
    assert np.array_equal(got, want), (n, C_, int((got != want).sum()))


# ---- b. update at several iterations per wavefront ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C_", K.TABLE, ids=IDS)
def test_update_at_several_iterations(n, C_):
    """the order contract of test_gpu_rbstats.test_order_contract_against_chainstats and the bounds of
    test_fields_against_longdouble; a low-rank term of rank 3 on the cases of RANKED"""
    import torch

    from parmgmc_amd import ChainStats

    lprl, chunks, iters, nb, rpw = K.geometry(n, C_)
    assert iters >= 2
    M = matrix(n)
    lr = R.lowrank(n, 3 if (n, C_) in K.RANKED else 0, seed=5)
    b = R.rhs(n, seed=3 * C_)
    steps = [R.samples(n, C_, seed=7 * C_ + s) for s in range(K.STEPS)]
    sd = [dev(Y) for Y in steps]
    rb = make_rb(M, C_, lr, b)
    cs = ChainStats(n, C_, [], max_steps=K.STEPS)
    for Y in sd:
        cs.update(rb.cond_mean(Y))
        rb.update(Y)
    assert rb.count() == (K.STEPS, K.STEPS * C_)
    mean, var = rb.fields()
    cmean, cvar = cs.fields()
    q = K.cond_precision_fast(M, lr)
    assert torch.equal(mean, cmean)
    assert np.array_equal(host(var), 1.0 / q + host(cvar))
    refs = [K.cond_mean_ref_fast(M, Y, b, lr) for Y in steps]
    check_fields(host(mean), host(var), refs, q, f"n={n} C={C_} LPRL={lprl} chunks={chunks} iters={iters}")
    if (n, C_) in K.TWICE:
        torch.cuda.synchronize()
        rb.reset()
        assert rb.count() == (0, 0)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            for Y in sd:
                rb.update(Y)
            mean2, var2 = rb.fields()
        st.synchronize()
        assert torch.equal(mean, mean2) and torch.equal(var, var2)


# ---- c. the cap ----------------------------------------------------------------------------------------------------------------------
def test_iteration_cap_of_chunked_chains():
    import torch

    from parmgmc_amd import ChainStats

    n, C_ = K.CAP_CASE
    lprl, chunks, iters, nb, rpw = K.geometry(n, C_)
    assert (lprl, chunks, iters, nb, rpw) == (6, 2, K.MAXRPW, 2049, 256) and K.uncapped_iters(n, C_) > K.MAXRPW and nb > K.MAXBLK
    steps_n = 2
    rng = np.random.default_rng(5)
    regions = -(-n // rpw)
    picked = []
    for reg in (0, regions // 2, regions - 2):  # whole wavefront regions: the first and the last row, it = 0, 1, 255
        base = reg * rpw
        picked += [base, base + rpw - 1] + [base + it for it in (0, 1, K.MAXRPW - 1)]
    picked += [(regions - 1) * rpw, n - 1] + list(range(n - 64, n)) + list(rng.integers(0, n, 4000))
    rows_h = np.unique(np.clip(picked, 0, n - 1))
    assert 3500 <= len(rows_h) <= 4100 and (regions - 1) * rpw == n - 1  # the last wavefront has one live row
    rows = torch.as_tensor(rows_h, device="cuda")

    Mi = K.build(n, integer=True)
    q = K.cond_precision_fast(Mi)
    gen = torch.Generator(device="cuda").manual_seed(11)
    bd = torch.randint(-8, 9, (n,), device="cuda", dtype=torch.float64, generator=gen)
    b_h = host(bd)
    rb = make_rb(Mi, C_)
    rb.set_rhs(bd)
    assert np.array_equal(rb.cond_precision(), q)
    cs = ChainStats(n, C_, [], max_steps=steps_n)

    # the matrix restated on the device: entry j of row i has the value INT_VALUES[int_value_index(i, j)] and column i + shifts[j]
    i = torch.arange(n, device="cuda")
    lens = torch.as_tensor(K.LENGTHS, device="cuda")[i % len(K.LENGTHS)]
    table = torch.as_tensor(K.INT_VALUES, device="cuda")
    sh = K.shifts(n)
    qd = dev(q)

    def exact(Y):
        s = torch.zeros_like(Y)
        for j in range(K.MAXLEN):
            a = torch.where(lens > j, table[K.int_value_index(i, j)], 0.0)
            s += a[:, None] * torch.roll(Y, -int(sh[j]), 0)  # row i of the shifted copy is row (i + shifts[j]) mod n of Y
        assert float(s.abs().max()) < 2**40  # integers far below 2^53: every sum is exact in any order
        return (bd[:, None] - s) / qd[:, None]  # a power of two divides

    refs = []
    for _ in range(steps_n):
        Y = torch.randint(-8, 9, (n, C_), device="cuda", dtype=torch.float64, generator=gen)
        got = rb.cond_mean(Y)
        want = exact(Y)
        assert torch.equal(got, want), int((got != want).sum())
        assert float(want.abs().max()) > 0
        del want
        cs.update(got)
        rb.update(Y)
        refs.append(K.cond_mean_ref_fast(Mi, None, b_h[rows_h], rows=rows_h, take=lambda c: host(Y[torch.as_tensor(c, device="cuda")])))
        assert np.array_equal(host(got[rows]).astype(np.longdouble), refs[-1][0])  # the two references agree on the picked rows
        del Y, got
    mean, var = rb.fields()
    cmean, cvar = cs.fields()
    assert torch.equal(mean, cmean)
    assert np.array_equal(host(var), 1.0 / q + host(cvar))
    check_fields(host(mean[rows]), host(var[rows]), refs, q[rows_h], f"cap n={n} C={C_} iters={iters} blocks={nb}, {len(rows_h)} rows")
    torch.cuda.synchronize()
    del rb, cs, mean, var, cmean, cvar
    torch.cuda.empty_cache()


# ---- d. negative controls ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C_", K.NEGATIVE)
def test_one_change_is_seen_where_it_belongs(n, C_):
    """tests/test_rbstats_geometry_cases.py asserts that the references move by at least 100 bounds at the rows and chains named
    here, and nowhere else"""
    ctl = K.controls(n, C_)
    lprl, chunks, iters, nb, rpw = K.geometry(n, C_)
    assert iters == 2 and (ctl.r % rpw) // (64 >> lprl) == 1 and ctl.r in ctl.rows_y and ctl.chain // 64 == chunks - 1
    T = len(ctl.steps)

    def run(M, steps):
        rb = make_rb(M, C_, None, ctl.b)
        ms = []
        for Y in steps:
            Yd = dev(Y)
            ms.append(host(rb.cond_mean(Yd)))
            rb.update(Yd)
        return ms, tuple(host(t) for t in rb.fields())

    refs = [K.cond_mean_ref_fast(ctl.M, Y, ctl.b) for Y in ctl.steps]
    m_ref, v_ref, mean_bound, var_bound = R.fields_reference([r[0] for r in refs], [r[1] for r in refs], ctl.q)
    m0, (mean0, var0) = run(ctl.M, ctl.steps)
    for t in range(T):
        assert (np.abs(m0[t] - refs[t][0]) <= refs[t][1]).all()
    assert (np.abs(mean0 - m_ref) <= mean_bound).all() and (np.abs(var0 - v_ref) <= var_bound).all()
    for what, M1, steps1, rows, chains in (("sample", ctl.M, ctl.steps_y, ctl.rows_y, [ctl.chain]), ("entry", ctl.M_a, ctl.steps, np.array([ctl.r]), list(range(C_)))):
        m1, (mean1, var1) = run(M1, steps1)
        for t in range(T):
            hit = np.zeros((n, C_), bool)
            if what == "entry" or t == T - 1:  # the sample is changed in the last step only
                hit[np.ix_(rows, chains)] = True
            assert np.array_equal(m1[t][~hit], m0[t][~hit]), (what, t)
            off = np.abs(m1[t] - refs[t][0])[hit] / refs[t][1][hit]
            assert (off > 1).all(), (what, t, float(off.min()) if off.size else None)
        others = np.ones(n, bool)
        others[rows] = False
        assert np.array_equal(mean1[others], mean0[others]) and np.array_equal(var1[others], var0[others]), what
        e_m, e_v = np.abs(mean1 - m_ref)[rows] / mean_bound[rows], np.abs(var1 - v_ref)[rows] / var_bound[rows]
        print(f"n={n} C={C_} changed {what}: {len(rows)} rows; m off by at least {float(off.min()):.3e} bounds, mean by {float(e_m.min()):.3e}, var by {float(e_v.min()):.3e}")
        assert (e_m > 1).all() and (e_v > 1).all(), (what, float(e_m.min()), float(e_v.min()))
