"""The Woodbury term through the C-ABI alone (pmg_woodbury_create with ldb, set_c_column / column, finish, get_correction,
noisy_rhs, correct and their _chains forms) against the extended-precision reference and the per-entry bounds of
tests/woodbury_cases.py, on every case of its table: one row to 65 blocks of 4096 rows, k = 1 .. 64, sqrt|S| of a negative
S, an unsymmetric T whose inverse has to pivot, ldb > n with NaN pad rows.  Then the chains forms against the single-chain
calls, bit for bit, at every chain count of the table (every lane split LPRL = 0 .. 6 of lrc_btx_chains_kernel<16, false, *>,
every chunk edge), with one column per case against the reference as well; negative controls on host copies of the device
results; the argument and state checks that need a handle.

The correction y' = y - G (B^T y) is checked twice: against the reference's own G, and with the bound evaluated on the G the
handle holds (read back; G itself is checked against the reference within its own bound)."""
import ctypes as C

import numpy as np
import pytest

import woodbury_cases as W

pytestmark = pytest.mark.gpu
ARG_NULL, ARG_OUTOFRANGE, ARG_WRONGSTATE, ERR_LIB = 85, 63, 73, 76
IDS = [W.case_id(c) for c in W.CASES]
ALL_COUNTS = sorted(W.CHAINS + W.CONTROLS)
MAXC = max(ALL_COUNTS)
BORROWED = W.Case(4097, 9, False, True, False)  # this case hands C over through pmg_woodbury_column's pointers


def dev(a):
    import torch

    return torch.as_tensor(np.array(a, np.float64), device="cuda")  # a copy: the inputs are read-only arrays


def _api():
    from parmgmc_amd.capi import check, lib
    from parmgmc_amd.wrappers import _ptr, _stream

    return lib, check, _ptr, _stream


def _memcpy(dst, src, nbytes, kind):
    """hipMemcpy of the runtime this process already uses, for the borrowed device pointers of pmg_woodbury_column (2: device
    to host, 3: device to device)"""
    hip = C.CDLL(None)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(dst, src, nbytes, kind) == 0


def make_handle(I, borrowed=False, finish=True):
    """create from the host image of B (ldb >= n), hand over the columns of C, finish"""
    import torch

    lib, check, _ptr, _stream = _api()
    h = C.c_void_p()
    check(lib.pmg_woodbury_create(I.n, I.k, I.B_host.ctypes.data, I.ldb, I.S.ctypes.data, None, C.byref(h)))
    for c in range(I.k):
        x = dev(I.C[:, c])
        if borrowed:
            check(lib.pmg_woodbury_set_c_column(h, c, _ptr(dev(np.full(I.n, 7.0))), _stream()))  # what the zero fill has to wipe
            bp, cp = C.c_void_p(), C.c_void_p()
            check(lib.pmg_woodbury_column(h, c, C.byref(bp), C.byref(cp), _stream()))
            got = np.full(I.n, np.nan)
            _memcpy(got.ctypes.data, cp, 8 * I.n, 2)
            assert not got.any(), "the C column is not zero-filled"
            _memcpy(got.ctypes.data, bp, 8 * I.n, 2)
            assert np.array_equal(got, I.B[:, c]), "the borrowed B column"
            _memcpy(cp, _ptr(x), 8 * I.n, 3)
        else:
            check(lib.pmg_woodbury_set_c_column(h, c, _ptr(x), _stream()))
    torch.cuda.synchronize()
    if finish:
        check(lib.pmg_woodbury_finish(h))
    return h


def get_correction(h, n, k):
    lib, check, _, _ = _api()
    G = np.full((n, k), np.nan, order="F")
    check(lib.pmg_woodbury_get_correction(h, G.ctypes.data))
    return G


def noisy_rhs(h, b_dev, seed, counter):
    import torch

    lib, check, _ptr, _stream = _api()
    w = torch.full_like(b_dev, float("nan"))
    check(lib.pmg_woodbury_noisy_rhs(h, _ptr(b_dev), _ptr(w), seed, counter, _stream()))
    return w


def correct(h, y_dev):
    lib, check, _ptr, _stream = _api()
    y = y_dev.clone()
    check(lib.pmg_woodbury_correct(h, _ptr(y), _stream()))
    return y


def noisy_rhs_chains(h, b_dev, seeds, counter):
    import torch

    lib, check, _ptr, _stream = _api()
    s = np.ascontiguousarray(seeds, np.uint64)
    Wd = torch.full((b_dev.shape[0], len(s)), float("nan"), dtype=torch.float64, device="cuda")
    check(lib.pmg_woodbury_noisy_rhs_chains(h, len(s), s.ctypes.data, counter, _ptr(b_dev), _ptr(Wd), _stream()))
    return Wd


def correct_chains(h, Y_dev):
    lib, check, _ptr, _stream = _api()
    Y = Y_dev.clone()
    check(lib.pmg_woodbury_correct_chains(h, Y.shape[1], _ptr(Y), _stream()))
    return Y


def destroy(h):
    lib, check, _, _ = _api()
    check(lib.pmg_woodbury_destroy(C.byref(h)))
    assert not h.value


# ---- every case of the table against the reference -------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.CASES, ids=IDS)
def test_term_against_the_reference(case):
    I, R = W.inputs(case), W.reference(case)
    seed, counter = W.noise_key(case)
    h = make_handle(I, borrowed=case == BORROWED)
    try:
        G = get_correction(h, I.n, I.k)
        w = noisy_rhs(h, dev(I.b), seed, counter).cpu().numpy()
        y1 = correct(h, dev(I.y)).cpu().numpy()
    finally:
        destroy(h)
    w_ref, wb = W.noisy_rhs_ref(R, I.b, seed, counter)
    y_ref, yb = W.correct_ref(R, I.y)
    y_refg, ybg = W.correct_ref(R, I.y, G=G)
    ratios = dict(G=W.g_ratio(G, R) if np.isfinite(G).all() else float("inf"), w=W.excess(w, w_ref, wb), y=W.excess(y1, y_ref, yb), y_with_G_held=W.excess(y1, y_refg, ybg))
    print(f"WOODBURY_RATIOS {W.case_id(case)} cond {R.cond:.1f} " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert np.isfinite(G).all() and np.isfinite(w).all() and np.isfinite(y1).all(), "a NaN reached an output (the pad rows?)"
    assert ratios["G"] <= W.G_MARGIN, ratios
    assert ratios["w"] <= 1.0, ratios
    assert ratios["y_with_G_held"] <= 1.0, ratios
    assert ratios["y"] <= 1.0, ratios
    # negative controls on the host copies: a row left out of B^T y, the last entry of S doubled
    r = W.heaviest_row(R, I.y)
    yd, ybd = W.correct_ref(R, I.y, drop_row=r)
    ydg, ybdg = W.correct_ref(R, I.y, G=G, drop_row=r)
    assert W.excess(y1, yd, ybd) > 1.0 and W.excess(y1, ydg, ybdg) > 1.0
    S2 = I.S.copy()
    S2[-1] *= 2.0
    R2 = W.build(I.B, I.C, S2)
    w2, wb2 = W.noisy_rhs_ref(R2, I.b, seed, counter)
    assert W.excess(w, w2, wb2) > 1.0 and W.g_ratio(G, R2) > W.G_MARGIN


# ---- chains against single-chain, bit for bit ------------------------------------------------------------------------------
_SHAPES = {}


def _shape(n, k, maxc=MAXC):
    """one finished handle per shape, the shared b, MAXC columns of Y and seeds, and the single-chain result of every column"""
    import torch

    if (n, k) not in _SHAPES:
        case = W.chain_case(n, k)
        I = W.inputs(case)
        h = make_handle(I)
        rng = np.random.default_rng(n + k)
        seeds = W.chain_seeds(maxc)
        counter = W.noise_key(case)[1]
        b = dev(I.b)
        Y0h = rng.standard_normal((n, maxc))
        Y0h[:, 0] = I.y
        Y0 = dev(Y0h)
        Ws = torch.stack([noisy_rhs(h, b, seeds[c], counter) for c in range(maxc)], 1)
        Ys = torch.stack([correct(h, Y0[:, c].contiguous()) for c in range(maxc)], 1)
        _SHAPES[(n, k)] = dict(case=case, I=I, h=h, seeds=seeds, counter=counter, b=b, Y0=Y0, Y0h=Y0h, Ws=Ws, Ys=Ys, G=get_correction(h, n, k))
    return _SHAPES[(n, k)]


def _chains_equal_single(s, nchains, against_reference=True):
    import torch

    Wd = noisy_rhs_chains(s["h"], s["b"], s["seeds"][:nchains], s["counter"])
    Yd = correct_chains(s["h"], s["Y0"][:, :nchains].contiguous())
    for c in range(nchains):
        assert torch.equal(Wd[:, c], s["Ws"][:, c]), ("noisy_rhs", nchains, c)
        assert torch.equal(Yd[:, c], s["Ys"][:, c]), ("correct", nchains, c)
    assert np.array_equal(s["b"].cpu().numpy(), s["I"].b), "b changed"
    if against_reference:  # the last chain: the last live lane of the last chunk
        c, R = nchains - 1, W.reference(s["case"])
        w_ref, wb = W.noisy_rhs_ref(R, s["I"].b, s["seeds"][c], s["counter"])
        assert W.excess(Wd[:, c].cpu().numpy(), w_ref, wb) <= 1.0
        y_ref, yb = W.correct_ref(R, s["Y0h"][:, c], G=s["G"])
        assert W.excess(Yd[:, c].cpu().numpy(), y_ref, yb) <= 1.0
        yd, ybd = W.correct_ref(R, s["Y0h"][:, c], G=s["G"], drop_row=W.heaviest_row(R, s["Y0h"][:, c]))
        assert W.excess(Yd[:, c].cpu().numpy(), yd, ybd) > 1.0


@pytest.mark.parametrize("nchains", ALL_COUNTS)
@pytest.mark.parametrize("n,k", W.CHAIN_SHAPES, ids=[f"n{n}-k{k}" for n, k in W.CHAIN_SHAPES])
def test_chains_equal_single_chain(n, k, nchains):
    """the counts ascend on one handle per shape: woodbury_chains_workspace grows at every new count"""
    _chains_equal_single(_shape(n, k), nchains)


@pytest.mark.parametrize("nchains", W.CHAIN_WRAP_COUNTS)
def test_chains_equal_single_chain_65_blocks(nchains):
    n, k = W.CHAIN_WRAP_SHAPE
    _chains_equal_single(_shape(n, k, max(W.CHAIN_WRAP_COUNTS)), nchains)


def test_one_handle_from_the_largest_count_down_and_up_again():
    """a fresh handle: the workspace is sized by the largest count and then reused by every smaller one (the block sums are
    nblocks x k x C, so a smaller C packs them differently into the same buffer); then a second fresh handle from the smallest
    up, which grows at every step, against the same single-chain columns"""
    s = dict(_shape(4097, 5))
    for order in (sorted(ALL_COUNTS, reverse=True) + ALL_COUNTS, ALL_COUNTS):
        s["h"] = make_handle(s["I"])
        try:
            for nchains in order:
                _chains_equal_single(s, nchains, against_reference=False)
        finally:
            destroy(s["h"])


@pytest.fixture(scope="module", autouse=True)
def _release_shared_handles():
    yield
    while _SHAPES:
        destroy(_SHAPES.popitem()[1]["h"])


# ---- argument and state checks that need a handle --------------------------------------------------------------------------
def test_state_checks():
    lib, check, _ptr, _stream = _api()
    I = W.inputs(W.Case(63, 5, False, True, False))
    h = make_handle(I, finish=False)
    y, G = dev(I.y), np.zeros((I.n, I.k), order="F")
    bp, cp = C.c_void_p(), C.c_void_p()
    seeds = np.arange(3, dtype=np.uint64)
    Y = dev(np.zeros((I.n, 3)))
    try:
        assert lib.pmg_woodbury_correct(h, _ptr(y), _stream()) == ARG_WRONGSTATE
        assert b"pmg_woodbury_finish" in lib.pmg_last_error_string()
        assert lib.pmg_woodbury_get_correction(h, G.ctypes.data) == ARG_WRONGSTATE
        assert lib.pmg_woodbury_correct_chains(h, 3, _ptr(Y), _stream()) == ARG_WRONGSTATE
        for c in (-1, I.k):
            assert lib.pmg_woodbury_set_c_column(h, c, _ptr(y), _stream()) == ARG_OUTOFRANGE
            assert lib.pmg_woodbury_column(h, c, C.byref(bp), C.byref(cp), _stream()) == ARG_OUTOFRANGE
        assert lib.pmg_woodbury_set_c_column(h, 0, None, _stream()) == ARG_NULL
        assert lib.pmg_woodbury_column(h, 0, None, C.byref(cp), _stream()) == ARG_NULL
        check(lib.pmg_woodbury_finish(h))
        assert lib.pmg_woodbury_finish(h) == ARG_WRONGSTATE
        assert lib.pmg_woodbury_set_c_column(h, 0, _ptr(y), _stream()) == ARG_WRONGSTATE
        assert lib.pmg_woodbury_column(h, 0, C.byref(bp), C.byref(cp), _stream()) == ARG_WRONGSTATE
        assert b"already built" in lib.pmg_last_error_string()
        for bad in (0, -3):
            assert lib.pmg_woodbury_noisy_rhs_chains(h, bad, seeds.ctypes.data, 0, _ptr(y), _ptr(Y), _stream()) == ARG_OUTOFRANGE
            assert lib.pmg_woodbury_correct_chains(h, bad, _ptr(Y), _stream()) == ARG_OUTOFRANGE
        assert lib.pmg_woodbury_noisy_rhs_chains(h, 3, None, 0, _ptr(y), _ptr(Y), _stream()) == ARG_NULL
        assert lib.pmg_woodbury_noisy_rhs_chains(h, 3, seeds.ctypes.data, 0, None, _ptr(Y), _stream()) == ARG_NULL
        assert lib.pmg_woodbury_correct_chains(h, 3, None, _stream()) == ARG_NULL
        assert lib.pmg_woodbury_correct(h, None, _stream()) == ARG_NULL
        assert lib.pmg_woodbury_noisy_rhs(h, None, _ptr(y), 1, 2, _stream()) == ARG_NULL
        assert lib.pmg_woodbury_get_correction(h, None) == ARG_NULL
        # the failed calls left the handle as it was
        R = W.reference(W.Case(63, 5, False, True, False))
        assert W.g_ratio(get_correction(h, I.n, I.k), R) <= W.G_MARGIN
    finally:
        destroy(h)


def test_exactly_singular_t_is_reported_and_the_handle_destroys():
    """k = 1: B = C = (1, 1), S = -1/2, so B^T C = 2 = -1/S and T = 0 in exact arithmetic of small integers"""
    import torch

    lib, check, _ptr, _stream = _api()
    B, S = np.ones((2, 1), order="F"), np.array([-0.5])
    h = C.c_void_p()
    check(lib.pmg_woodbury_create(2, 1, B.ctypes.data, 2, S.ctypes.data, None, C.byref(h)))
    check(lib.pmg_woodbury_set_c_column(h, 0, _ptr(dev(np.ones(2))), _stream()))
    torch.cuda.synchronize()
    assert lib.pmg_woodbury_finish(h) == ERR_LIB
    assert b"singular" in lib.pmg_last_error_string()
    assert lib.pmg_woodbury_correct(h, _ptr(dev(np.ones(2))), _stream()) == ARG_WRONGSTATE  # not finished
    destroy(h)
    # one unit away it is regular: T = 1/S + 2 with S = -1 gives G = C / 1
    S = np.array([-1.0])
    check(lib.pmg_woodbury_create(2, 1, B.ctypes.data, 2, S.ctypes.data, None, C.byref(h)))
    check(lib.pmg_woodbury_set_c_column(h, 0, _ptr(dev(np.ones(2))), _stream()))
    torch.cuda.synchronize()
    check(lib.pmg_woodbury_finish(h))
    assert np.array_equal(get_correction(h, 2, 1), np.ones((2, 1)))
    destroy(h)


def test_no_rows_on_one_device():
    """n = 0 (an empty rank's share, here alone): every call works and T = S^-1 is inverted"""
    import torch

    lib, check, _ptr, _stream = _api()
    S = np.array([30.0, -40.0, 50.0])
    h = C.c_void_p()
    check(lib.pmg_woodbury_create(0, 3, None, 0, S.ctypes.data, None, C.byref(h)))
    bp, cp = C.c_void_p(), C.c_void_p()
    check(lib.pmg_woodbury_column(h, 0, C.byref(bp), C.byref(cp), _stream()))
    for c in range(3):
        check(lib.pmg_woodbury_set_c_column(h, c, None, _stream()))
    check(lib.pmg_woodbury_finish(h))
    G = np.full(4, 3.0)
    check(lib.pmg_woodbury_get_correction(h, G.ctypes.data))
    assert (G == 3.0).all()  # nothing to copy
    check(lib.pmg_woodbury_noisy_rhs(h, None, None, 1, 2, _stream()))
    check(lib.pmg_woodbury_correct(h, None, _stream()))
    seeds = np.arange(5, dtype=np.uint64)
    check(lib.pmg_woodbury_noisy_rhs_chains(h, 5, seeds.ctypes.data, 2, None, None, _stream()))
    check(lib.pmg_woodbury_correct_chains(h, 5, None, _stream()))
    torch.cuda.synchronize()
    destroy(h)
