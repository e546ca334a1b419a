"""The IACT of every chain on the device (pmg_iact_chains, pmg_chainstats_iact) against the extended-precision restatement of
its semantics (iact_cases.truth) and the host path pmg_iact.

Bounds, from the input alone (iact_cases.rho_bound / tau_bound):  |rho_dev[k] - rho_ld[k]| <= 8 n 2^-53 (1 + |mean| / rms(z)),
|tau_dev - tau_ld| <= 2 (window + 1) times that; windows and valid flags equal the host's exactly.  Every fixture keeps
|i - 5 T_i| > 1e-6 for i <= window on the host values: asserted, since the window is a discrete decision.
Every comparison prints its figures (pytest -s) before it asserts."""
import numpy as np
import pytest

import iact_cases as K
import oracle as O

pytestmark = pytest.mark.gpu
ARG_OUTOFRANGE = 63


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def lag_block():
    from parmgmc_amd import IACT_LAG_BLOCK

    return IACT_LAG_BLOCK


def host_all(x):
    """host_iact of every column, with the fixture precondition"""
    out = [K.host_iact(x[:, s]) for s in range(x.shape[1])]
    for s, (tau, w, v, T) in enumerate(out):
        if not np.isnan(tau):
            assert K.margin(T, w) > K.MARGIN, (s, w, K.margin(T, w))  # a wrong fixture, not a wrong kernel
    return out


def check(x, got, label, host=None, nacf=0):
    """device results of the columns of x against the host's windows / flags and the long-double tau (and rho with nacf > 0)"""
    tau, window, valid = got[:3]
    host = host or host_all(x)
    worst_t = worst_r = 0.0
    for s, (htau, hw, hv, _) in enumerate(host):
        assert window[s] == hw and bool(valid[s]) == hv, (label, s, int(window[s]), hw, bool(valid[s]), hv)
        rho, T = K.truth(x[:, s], max(hw + 1, nacf))
        err, bound = abs(float(tau[s] - T[hw])), K.tau_bound(x[:, s], hw)
        worst_t = max(worst_t, err / bound)
        assert err <= bound, (label, s, err, bound)
        if nacf:
            acf = got[3][:, s].cpu().numpy()
            err, bound = float(np.abs(acf - rho[:nacf]).max()), K.rho_bound(x[:, s])
            worst_r = max(worst_r, err / bound)
            assert err <= bound, (label, s, err, bound)
    print(f"{label}: windows {min(h[1] for h in host)}..{max(h[1] for h in host)}, worst tau err / bound {worst_t:.3e}" + (f", worst rho err / bound {worst_r:.3e}" if nacf else ""))
    return host


@pytest.mark.parametrize("n,S", [(2, 1), (3, 2), (257, 3), (1000, 64), (4097, 65)])
def test_ar1_matrices(n, S):
    from parmgmc_amd import iact_chains

    x = K.ar1_cycle(n, S, 1234 + n)
    check(x, iact_chains(dev(x)), f"AR(1) n={n} S={S}")


def test_long_windows():
    """several lag blocks: host windows 93, 339, 1317"""
    from parmgmc_amd import iact_chains

    x = K.ar1(20000, [0.9, 0.97, 0.99], np.random.default_rng(99))
    host = check(x, iact_chains(dev(x)), "long windows")
    assert [h[1] for h in host] == [93, 339, 1317]


def edge_series():
    """(target window, series) around the edges of a lag block"""
    LB = lag_block()
    out = []
    for w in (LB - 1, LB, LB + 1, 2 * LB):
        n, seed = K.EDGE_SEEDS[w]
        out.append((w, K.ar1(n, [K.phi_for_window(w)], np.random.default_rng(seed))[:, 0]))
    return out


def test_lag_block_edges():
    from parmgmc_amd import iact_chains

    for w, x in edge_series():
        host = check(x[:, None], iact_chains(dev(x[:, None])), f"block edge {w}")
        assert host[0][1] == w, (host[0][1], w)


def test_offset_series():
    """100 + AR(1): the |mean| / rms term of the bound"""
    from parmgmc_amd import iact_chains

    x = 100.0 + K.ar1(1000, [0.5, 0.9], np.random.default_rng(7))
    host = check(x, iact_chains(dev(x)), "offset 100")
    assert [h[1] for h in host] == [13, 78]


def test_max_lag():
    from parmgmc_amd import iact_chains

    x = np.ascontiguousarray(K.ar1(20000, [0.9, 0.97, 0.99], np.random.default_rng(99))[:, :2])  # two series of test_long_windows
    X = dev(x)
    host = host_all(x)
    ws = [h[1] for h in host]
    assert ws == [93, 339]
    tau0, win0, val0 = iact_chains(X)
    assert list(win0) == ws
    for ml in (ws[1], ws[1] + 1, 19999, 20000, 1 << 30):  # the largest window and above: the unlimited call bit for bit
        tau, win, val = iact_chains(X, max_lag=ml)
        assert np.array_equal(tau, tau0) and np.array_equal(win, win0) and np.array_equal(val, val0), ml
    for ml in (ws[0] - 1, ws[0], 1, 300):  # below one or both windows
        tau, win, val = iact_chains(X, max_lag=ml)
        for s in range(2):
            if ml >= ws[s]:
                assert tau[s] == tau0[s] and win[s] == win0[s] and val[s] == val0[s], (ml, s)
                continue
            _, T = K.truth(x[:, s], ml + 1)
            err, bound = abs(float(tau[s] - T[ml])), K.tau_bound(x[:, s], ml)
            print(f"max_lag {ml} series {s}: tau err {err:.3e} / bound {bound:.3e}")
            assert win[s] == -1 and not val[s], (ml, s, win[s], val[s])
            assert err <= bound, (ml, s, err, bound)


def test_constant_series():
    from parmgmc_amd import iact_chains

    n = 600
    x = np.stack([np.full(n, 3.25), K.ar1(n, [0.5], np.random.default_rng(5))[:, 0], np.zeros(n)], axis=1)
    got = iact_chains(dev(x), nacf=4)
    tau, win, val, acf = got
    htau, hw, hv, _ = K.host_iact(x[:, 2])
    assert np.isnan(htau) and hw == n - 1 and not hv  # what the host gives for c_0 = 0
    for s in (0, 2):  # 3.25 k is exact for k <= 600: the device mean is 3.25 and c_0 = 0 there too
        assert np.isnan(tau[s]) and win[s] == n - 1 and not val[s], (s, tau[s], win[s], val[s])
        assert bool(acf[:, s].isnan().all())
    sub = (tau[1:2], win[1:2], val[1:2], acf[:, 1:2])
    check(x[:, 1:2], sub, "beside constant series", nacf=4)


def test_acf_output():
    """nacf beyond the window makes the scan go on to nacf; tau and window do not change"""
    from parmgmc_amd import iact_chains

    n = 257
    x = K.ar1_cycle(n, 3, 1234 + n)
    X = dev(x)
    base = iact_chains(X)
    host = host_all(x)
    assert max(h[1] for h in host) < lag_block()
    for nacf in (1, lag_block() + 1, n):
        got = iact_chains(X, nacf=nacf)
        assert tuple(got[3].shape) == (nacf, 3)
        for a, b in zip(got[:3], base):
            assert np.array_equal(a, b), nacf
        check(x, got, f"acf nacf={nacf}", host=host, nacf=nacf)
        assert bool((got[3][0] == 1.0).all())


def test_column_slice():
    """ld > S: the call on a column slice of a wider tensor"""
    import torch

    from parmgmc_amd import iact_chains

    n, S = 1000, 5
    x = K.ar1_cycle(n, S, 77)
    wide = torch.full((n, S + 6), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, 2 : 2 + S] = dev(x)
    view = wide[:, 2 : 2 + S]
    assert not view.is_contiguous()
    got = iact_chains(view, nacf=20)
    check(x, got, "column slice", nacf=20)
    ref = iact_chains(dev(x), nacf=20)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and torch.equal(got[3], ref[3])


@pytest.mark.parametrize("C", [3, 65])
def test_chainstats_traces(C):
    """traces that are known AR(1) series: Y[r, c] = x[s, c] / n_rows, an all-ones and a weighted QOI"""
    import torch

    from parmgmc_amd import ChainStats, PMGError

    n_rows, steps, first = 8, 600, 5
    x = K.ar1_cycle(steps, C, 4321 + C)
    wts = np.linspace(0.5, 2.0, n_rows)
    cs = ChainStats(n_rows, C, [None, wts], max_steps=steps)
    X = dev(x)
    for s in range(steps):
        cs.update((X[s] / n_rows).expand(n_rows, C).contiguous())
    for q in (0, 1):
        for count in (None, 300):
            tr = cs.trace(q, first, count)
            hosted = cs.iact(q, first, count)
            host = host_all(tr)
            assert [(h[0], h[2]) for h in host] == hosted  # cs.iact is pmg_iact on these columns
            got = cs.iact_device(q, first, count, nacf=7)
            check(tr, got, f"ChainStats C={C} q={q} count={count}", host=host, nacf=7)
            assert np.array_equal(got[0], cs.iact_device(q, first, count)[0])
    # the checks a handle with recorded steps can reach
    for kw in ({"max_lag": -1}, {"nacf": 301, "count": 300}, {"q": 2}, {"first": steps - 1}, {"first": 1, "count": steps}):
        with pytest.raises(PMGError) as e:
            cs.iact_device(**kw)
        assert e.value.code == ARG_OUTOFRANGE, kw
    from parmgmc_amd.capi import lib

    tau, acf = np.empty(C), torch.empty((7, C), dtype=torch.float64, device="cuda")
    assert lib.pmg_chainstats_iact(cs._h, 0, 0, 300, 0, tau.ctypes.data, None, None, -1, acf.data_ptr(), None) == ARG_OUTOFRANGE
    assert lib.pmg_chainstats_iact(cs._h, 0, 0, 300, 0, tau.ctypes.data, None, None, -1, None, None) == 0  # no acf: nacf is ignored
    assert np.array_equal(tau, cs.iact_device(0, 0, 300)[0])
    torch.cuda.synchronize()


def test_same_bits_on_a_side_stream():
    import torch

    from parmgmc_amd import iact_chains

    x = K.ar1_cycle(1000, 64, 1234 + 1000)
    a = iact_chains(dev(x), nacf=300)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        X = dev(x) * 1.0  # produced on the side stream
        b = iact_chains(X, nacf=300)
    st.synchronize()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert torch.equal(a[3], b[3])
    c = iact_chains(dev(x), nacf=300)
    assert np.array_equal(a[0], c[0]) and torch.equal(a[3], c[3])


def test_mgmc_chains_end_to_end():
    """MGMC.sample_chains with stats= on the galerkin27 operator's aggregation hierarchy, 8 chains, 300 steps"""
    import torch

    from parmgmc_amd import MGMC, ChainStats
    from parmgmc_amd.unstructured import build_hierarchy

    A = O.CSR.from_scipy(O.galerkin(O.shifted_laplace(9, 9, 9, 1.0).scipy(), O.q1_interp(5, 5, 5)))
    ops, ps = build_hierarchy(A.scipy().tocsr(), coarse_max=40)
    mg = MGMC.from_hierarchy(ops, ps)
    mg.set_smoother(True, 1.0, 1, 1)
    mg.setup()
    n, C, steps = A.n, 8, 300
    rng = np.random.default_rng(8)
    cs = ChainStats(n, C, [None, rng.standard_normal(n)], max_steps=steps)
    b = dev(rng.standard_normal(n))
    Y = torch.zeros((n, C), dtype=torch.float64, device="cuda")
    mg.sample_chains(b, Y, steps, [0x1AC7 + 7919 * c for c in range(C)], stats=cs)
    assert cs.count() == (steps, steps * C)
    for q in (0, 1):
        tr = cs.trace(q, 5)
        host = host_all(tr)
        assert [(h[0], h[2]) for h in host] == cs.iact(q, 5)
        check(tr, cs.iact_device(q, 5), f"MGMC chains q={q}", host=host)
