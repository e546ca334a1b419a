"""The matrix-free Rao-Blackwellised statistics handle on a DMDA grid (pmg_rbstats_create_dmda, kernels_rbstats_dmda.hip) on the
device.  Its contract is the bits of the CSR handle on oracle.shifted_laplace of the same grid: unless said otherwise the
expected values below come from that handle and are compared with np.array_equal / torch.equal -- no tolerance.  The definition
itself is held by the np.longdouble reference and the forward-error bounds of tests/rbstats_cases.py, and by integer data on
which nothing rounds."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import rbstats_cases as R

pytestmark = pytest.mark.gpu
ARG_WRONGSTATE, ARG_SIZ = 73, 60
KAPPA = 0.7  # 0.7 * 0.7 rounds
PAD = 33  # doubles of sentinel on either side of Y; odd, so that Y itself starts 8-byte aligned only

# x lines below, at and across a wavefront, even and odd nx; 2-D grids; grids whose every point lies on a face (nz = 2, ny = 2);
# 17^3 and 33 x 33 x 5: more than one block per plane, and at 17^3 three plane ranges per block column, the last of one plane
GRIDS = [(2, 2, 1), (5, 4, 3), (9, 9, 1), (4, 4, 4), (6, 2, 5), (7, 6, 2), (64, 3, 2), (65, 3, 2), (66, 5, 3), (129, 2, 2), (130, 3, 1), (17, 17, 17), (33, 33, 5)]
# every lpr, a partial lane group, the chunk boundary and a partial last chunk, on the three smallest 3-D grids and 33 x 33 x 5
CHAIN_GRIDS = [(5, 4, 3), (4, 4, 4), (6, 2, 5), (33, 33, 5)]
CHAINS = [2, 3, 8, 9, 33, 64, 65, 130]
CASES = [(g, 1) for g in GRIDS] + [(g, c) for g in CHAIN_GRIDS for c in CHAINS]


def gid(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def assembled(grid, kappa=KAPPA):
    return O.shifted_laplace(*grid, kappa)


def matrix(grid, kappa=KAPPA):
    A = assembled(grid, kappa)
    return R.Matrix(gid(grid), A.rowptr, A.colidx, A.vals, A.n, "shifted_laplace")


def handles(grid, C_, lr=None, b=None, kappa=KAPPA):
    """(the DMDA handle, the CSR handle on the assembled operator), the same (B, S) and right-hand side on both"""
    from parmgmc_amd import RBStats

    bd = None if b is None else dev(b)
    return RBStats.dmda(*grid, kappa, C_, lowrank=lr, b=bd), RBStats(assembled(grid, kappa), C_, lowrank=lr, b=bd)


def guarded(Y):
    """(view, buffer): Y as a contiguous view that starts an odd number of doubles into a NaN-filled buffer"""
    import torch

    buf = torch.full((Y.numel() + 2 * PAD,), float("nan"), dtype=torch.float64, device="cuda")
    view = buf[PAD : PAD + Y.numel()].view(Y.shape)
    view.copy_(Y)
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view, buf


def same(x, y):
    import torch

    assert x.shape == y.shape and bool(torch.isfinite(y).all()) and torch.equal(x.view(torch.int64), y.view(torch.int64))


def geometry(grid, C_):
    from parmgmc_amd.capi import lib

    fn = lib.pmgk_rbstats_dmda_geometry
    fn.restype, fn.argtypes = None, [C.c_int32] * 4 + [C.POINTER(C.c_int32)] * 2
    it, nb = C.c_int32(), C.c_int32()
    fn(*grid, C_, C.byref(it), C.byref(nb))
    return it.value, nb.value


def check_against_csr(grid, C_, lr=None, seed=0):
    """cond_mean, the fields after three updates, reset, and the fields after two more; b random and NULL; Y between sentinels"""
    import torch

    n = int(np.prod(grid))
    steps = [R.samples(n, C_, seed=seed + 11 * s + C_) for s in range(5)]
    for b in (R.rhs(n, seed=seed + C_), None):
        dm, cs = handles(grid, C_, lr, b)
        views = [guarded(dev(Y)) for Y in steps]
        plain = [dev(Y) for Y in steps]
        same(dm.cond_mean(views[0][0]), cs.cond_mean(plain[0]))
        for t in range(3):
            dm.update(views[t][0])
            cs.update(plain[t])
        assert dm.count() == cs.count() == (3, 3 * C_)
        for x, y in zip(dm.fields(), cs.fields()):
            same(x, y)
        torch.cuda.synchronize()
        dm.reset(), cs.reset()
        for t in (3, 4):  # a fourth update; the fifth gives a single chain its second sample
            dm.update(views[t][0])
            cs.update(plain[t])
        for x, y in zip(dm.fields(), cs.fields()):
            same(x, y)
        for (view, buf), Y in zip(views, plain):  # the inputs and the sentinels are what they were
            assert torch.equal(view, Y) and bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + Y.numel() :]).all())


# ---- 6: the bits of the CSR handle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,C_", CASES, ids=[f"{gid(g)}-C{c}" for g, c in CASES])
def test_bits_of_the_csr_handle(grid, C_):
    check_against_csr(grid, C_, seed=sum(grid))


# ---- 7: the definition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [1, 3, 65])
@pytest.mark.parametrize("grid,k", [((5, 4, 3), 0), ((9, 9, 1), 3), ((17, 17, 17), 0), ((66, 5, 3), 1)], ids=gid)
def test_against_longdouble(grid, k, C_):
    """cond_mean within bound_m of rbstats_cases.cond_mean_ref, the fields of three updates within fields_reference's bounds"""
    M = matrix(grid)
    T = 3
    lr = R.lowrank(M.n, k, seed=5)
    b = R.rhs(M.n, seed=3 * C_)
    steps = [R.samples(M.n, C_, seed=7 * C_ + s) for s in range(T)]
    rb, _ = handles(grid, C_, lr, b)
    refs = [R.cond_mean_ref(M, Y, b, lr) for Y in steps]
    got = host(rb.cond_mean(dev(steps[0]))).reshape(M.n, C_)
    err = np.abs(got.astype(np.longdouble) - refs[0][0])
    print(f"{gid(grid)} k={k} C={C_}: worst cond_mean err / bound {float((err / refs[0][1]).max()):.3f}")
    assert np.isfinite(got).all() and (err <= refs[0][1]).all()
    for Y in steps:
        rb.update(dev(Y))
    mean, var = (host(t) for t in rb.fields())
    m_ref, v_ref, mean_bound, var_bound = R.fields_reference([r[0] for r in refs], [r[1] for r in refs], R.cond_precision_host(M, lr))
    mean_err, var_err = np.abs(mean - m_ref), np.abs(var - v_ref)
    print(f"  mean err / bound {float((mean_err / mean_bound).max()):.3e}; var err / bound {float((var_err / var_bound).max()):.3e}")
    assert (mean_err <= mean_bound).all() and (var_err <= var_bound).all()


# ---- 8: integer data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [1, 3, 65])
@pytest.mark.parametrize("grid", [(5, 4, 3), (9, 9, 1), (17, 5, 9), (129, 3, 2)], ids=gid)
def test_exact_on_integer_data(grid, C_):
    """nx = 2^p + 1 makes hinv2 a power of two and kappa = 0.5 makes kappa^2 one; with integer y and b the sum s, b - s and q
    are exact in any order, so m is the one correctly rounded quotient of two exact numbers: formed here from shifted copies of Y"""
    import torch

    nx, ny, nz = grid
    n = nx * ny * nz
    hinv2 = 1.0 / ((nx - 1) * (nx - 1))
    assert np.log2(hinv2) == int(np.log2(hinv2))
    Y = dev(R.samples(n, C_, seed=C_, integer=True)).view(nz, ny, nx, C_)
    b = R.rhs(n, seed=C_, integer=True)
    nb = torch.zeros_like(Y)
    cnt = torch.zeros((nz, ny, nx, 1), dtype=torch.float64, device="cuda")
    for axis in range(3):
        if Y.shape[axis] > 1:
            lo, hi = [slice(None)] * 4, [slice(None)] * 4
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            nb[tuple(hi)] += Y[tuple(lo)]
            nb[tuple(lo)] += Y[tuple(hi)]
            cnt[tuple(hi)] += 1
            cnt[tuple(lo)] += 1
    want = (dev(b).view(nz, ny, nx, 1) - (-hinv2) * nb) / (0.25 + hinv2 * cnt)
    rb, _ = handles(grid, C_, None, b, kappa=0.5)
    got = rb.cond_mean(Y.reshape(n, C_))
    assert torch.equal(got, want.reshape(n, C_))
    assert np.array_equal(rb.cond_precision(), host(0.25 + hinv2 * cnt).ravel())


# ---- 9: the launch geometry ----------------------------------------------------------------------------------------------------------
def smallest_cube(C_):
    """the smallest g^3 on which every wavefront takes two or more plane steps (C = 1) or row iterations and there is more
    than one workgroup, from the library's own geometry function"""
    for g in range(2, 200):
        it, nb = geometry((g, g, g), C_)
        if it >= 2 and nb > 1:
            return g
    raise AssertionError(C_)


# one chain per template instantiation of the chains kernel (lpr = 2 .. 64, and 65 for the chunked one) and the march kernel
GEOMETRY = {1: 9, 2: 65, 3: 51, 8: 41, 9: 33, 17: 26, 33: 21, 65: 21}


@pytest.mark.parametrize("C_", list(GEOMETRY))
def test_launch_geometry(C_):
    """one update and cond_mean (STORE and not) on the smallest cube with two or more steps per wavefront and more than one
    workgroup: 9^3 for the march (8 planes, then 1), 65^3 .. 21^3 for lpr = 2 .. 64 as for the CSR kernel (n / (4 G) > 2048)"""
    g = smallest_cube(C_)
    assert g == GEOMETRY[C_]
    grid = (g, g, g)
    n = g**3
    Y0, Y1 = (dev(R.samples(n, C_, seed=C_ + s)) for s in range(2))
    b = R.rhs(n, seed=C_)
    dm, cs = handles(grid, C_, None, b)
    same(dm.cond_mean(Y0), cs.cond_mean(Y0))
    for h in (dm, cs):
        h.update(Y0)
        h.update(Y1)
    for x, y in zip(dm.fields(), cs.fields()):
        same(x, y)


@pytest.mark.parametrize("grid", [(3, 2, 16400), (40, 40, 30), (17, 17, 17)], ids=gid)
def test_march_geometry(grid):
    """C = 1 where the block limit and not the minimum sets the planes per wavefront (3 x 2 x 16400: one block per plane, 9
    planes each), where a plane takes several blocks with a partial last one (40 x 40: 7 blocks, the last of 64 points), and
    with a last plane range of one plane (17^3)"""
    it, nb = geometry(grid, 1)
    nx, ny, nz = grid
    nbp = (nx * ny + 255) // 256
    assert nb == nbp * ((nz + it - 1) // it) and 1 <= it <= nz
    assert {(3, 2, 16400): it == 9 and nb == 1823, (40, 40, 30): it == 8 and nbp == 7 and nb == 28, (17, 17, 17): it == 8 and nb == 6}[grid]
    check_against_csr(grid, 1, seed=it)


@pytest.mark.parametrize("grid,C_", [((9, 9, 9), 1), ((21, 21, 21), 65), ((5, 4, 3), 3)], ids=gid)
def test_one_entry_moves_the_rows_that_read_it(grid, C_):
    """changing y at one point and chain changes m in exactly the in-domain neighbours of the point, in that chain -- the point's
    own m does not read its own y (without a low-rank term the row's sum runs over j != i)"""
    nx, ny, nz = grid
    n = nx * ny * nz
    Y = R.samples(n, C_, seed=4)
    rb, _ = handles(grid, C_, None, R.rhs(n, seed=1))
    base = host(rb.cond_mean(dev(Y))).reshape(n, C_)
    for i, j, k in [(0, 0, 0), (nx - 1, ny - 1, nz - 1), (nx // 2, ny // 2, nz // 2), (0, ny // 2, nz - 1), (nx - 1, 0, nz // 2)]:
        c = (i + j + k) % C_
        row = i + nx * (j + ny * k)
        Y2 = Y.copy()
        Y2[row, c] += 1.0
        got = host(rb.cond_mean(dev(Y2))).reshape(n, C_)
        moved = {tuple(x) for x in np.argwhere(got != base)}
        want = set()
        for d, (p, ext, stride) in enumerate([(i, nx, 1), (j, ny, nx), (k, nz, nx * ny)]):
            if p > 0:
                want.add((row - stride, c))
            if p < ext - 1:
                want.add((row + stride, c))
        assert moved == want, (i, j, k)


# ---- 10: the low-rank term -----------------------------------------------------------------------------------------------------------
def observation_lowrank(grid, k):
    """(B, S) of rank k: ball observations on the grid (pmg_make_observation_mats_dmda; the first ball is cut by the boundary),
    then random columns with a zero row"""
    from parmgmc_amd import make_observation_mats

    n = int(np.prod(grid))
    Bo, So, _ = make_observation_mats(*grid, [0.05, 0.1, 0.9, 0.6, 0.5, 0.45], [0.2, 0.22], [1.0, -2.0], 0.05)
    assert (Bo != 0).sum(axis=0).min() > 3 and (Bo[:, 0] != 0).sum() < (Bo[:, 1] != 0).sum()  # the first ball is cut
    rng = np.random.default_rng(k)
    Br = rng.uniform(-1.0, 1.0, (n, max(k - 2, 0))) / np.sqrt(n)
    B = np.concatenate([Bo[:, : min(k, 2)], Br], axis=1)
    B[n // 3] = 0.0
    S = np.concatenate([So[: min(k, 2)], rng.uniform(0.5, 20.0, max(k - 2, 0))])
    return np.asfortranarray(B), S


@pytest.mark.parametrize("C_", [1, 3, 65])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_lowrank_against_the_csr_handle(k, C_):
    grid = (17, 17, 17)
    lr = observation_lowrank(grid, k)
    check_against_csr(grid, C_, lr, seed=k)
    dm, cs = handles(grid, C_, lr)
    assert np.array_equal(dm.cond_precision(), cs.cond_precision())
    dm.set_lowrank(None)  # and the term goes away: the fields of the handle without one
    plain, _ = handles(grid, C_)
    Y = dev(R.samples(17**3, C_, seed=k))
    same(dm.cond_mean(Y), plain.cond_mean(Y))


# ---- 11: the wiring --------------------------------------------------------------------------------------------------------------------
def test_wiring_mgmc_sample():
    import torch

    from parmgmc_amd import MGMC, RBStats

    grid, its = (17, 17, 17), 6
    n = 17**3
    mg = MGMC(*grid, KAPPA, 3).setup()
    b = dev(R.rhs(n, seed=2))
    got = []
    y1 = torch.zeros(n, dtype=torch.float64, device="cuda")
    mg.sample(b, y1, its, seed=0xBEEF, callback=lambda it, y: got.append(y.clone()))
    assert len(got) == its
    rb = RBStats.dmda(*grid, KAPPA, b=b)
    y2 = torch.zeros_like(y1)
    mg.sample(b, y2, its, seed=0xBEEF, rb=rb)
    assert torch.equal(y1, y2)
    by_hand, csr = RBStats.dmda(*grid, KAPPA, b=b), RBStats(assembled(grid), 1, b=b)
    for y in got:
        by_hand.update(y)
        csr.update(y)
    assert rb.count() == by_hand.count() == (its, its)
    for x, y, z in zip(rb.fields(), by_hand.fields(), csr.fields()):
        same(x, y)
        same(x, z)
    with pytest.raises(AssertionError):  # the wrapper refuses other sizes before the library is called
        mg.sample(b, y2, 1, seed=1, rb=RBStats.dmda(17, 17, 16, KAPPA))


def test_wiring_grid_sample_loop_and_refusals():
    import torch

    from parmgmc_amd import GridMCSOR, PMGError, RBStats
    from parmgmc_amd.capi import lib

    grid, n = (9, 9, 1), 81
    g = GridMCSOR(*grid, KAPPA)
    b = dev(R.rhs(n, seed=9))
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    dm, cs = handles(grid, 1, None, host(b))
    ctr = 0
    for it in range(5):
        ctr = g.sample(b, y, 1, seed=77, counter0=ctr)
        dm.update(y)
        cs.update(y)
        if it == 0:  # one sample: src/ms.c:233
            with pytest.raises(PMGError) as e:
                dm.fields()
            assert e.value.code == ARG_WRONGSTATE
    for x, z in zip(dm.fields(), cs.fields()):
        same(x, z)
    # a z-slab's rows, another grid, other chains: refused by the library's callbacks, nothing recorded
    Y = C.c_void_p(y.data_ptr())
    other = RBStats.dmda(9, 9, 4, KAPPA, 2)
    assert lib.pmg_rbstats_callback(0, Y, 81 * 2, 2, other._h) == ARG_SIZ
    assert lib.pmg_rbstats_callback(0, Y, 81 * 4, 1, other._h) == ARG_SIZ
    assert lib.pmg_rbstats_sample_callback(0, Y, 81 * 4, other._h) == ARG_SIZ
    assert lib.pmg_rbstats_sample_callback(0, Y, 80, dm._h) == ARG_SIZ
    assert other.count() == (0, 0) and dm.count() == (5, 5)


# ---- 12: call history and streams ------------------------------------------------------------------------------------------------------
HISTORY = {"march": ((17, 17, 9), 1, 0), "chains_k3": ((9, 9, 5), 8, 3)}


@pytest.fixture(scope="module")
def hist():
    rng = np.random.default_rng(8)
    out = {}
    for case, (grid, C_, k) in HISTORY.items():
        n = int(np.prod(grid))
        lr = (np.asfortranarray(rng.uniform(-1.0, 1.0, (n, k)) / np.sqrt(n)), np.array([2.0, 5.0, 11.0])) if k else None
        out[case] = {"grid": grid, "C": C_, "lr": lr, "b": dev(rng.standard_normal(n)), "x": {f"Y{i}": dev(rng.standard_normal((n, C_))) for i in range(3)}, "alone": None}
    return out


def history_run(case, order, hist, between=None):
    """test_gpu_rbstats_history.run on a DMDA handle: {position: results} of the steps of `order` on one new handle"""
    import test_gpu_rbstats_history as HI
    import torch

    from parmgmc_amd import RBStats

    c = hist[case]
    rb, x = RBStats.dmda(*c["grid"], KAPPA, c["C"], lowrank=c["lr"], b=c["b"]), {k: v.clone() for k, v in c["x"].items()}
    out = []
    for i, name in enumerate(order):
        if between is not None and i:
            between(i, rb, x)
        out.append(HI.step(name, rb, x))
        torch.cuda.synchronize()
        for k, v in c["x"].items():
            assert HI.same_bits(x[k], v), f"step {name!r} left input {k!r} changed; call order: {order}"
    return out


def history_alone(case, hist):
    import test_gpu_rbstats_history as HI

    if hist[case]["alone"] is None:
        hist[case]["alone"] = {v: history_run(case, [v], hist)[0] for v in HI.VARIANTS}
    return hist[case]["alone"]


@pytest.mark.parametrize("case", list(HISTORY))
def test_history(case, hist):
    """every step alone gives the bits of the CSR handle; the steps in five orders, each step twice, and with a refused call in
    between give the bits of the step alone (the machinery of tests/test_gpu_rbstats_history.py)"""
    import handle_steps as H
    import test_gpu_rbstats_history as HI

    from parmgmc_amd import RBStats

    c = hist[case]
    want = history_alone(case, hist)
    twin = HI.step("cond_mean", RBStats(assembled(c["grid"]), c["C"], lowrank=c["lr"], b=c["b"]), c["x"])
    for name, out in want.items():
        assert out["count"] == (3, 3 * c["C"])
        for tag in ("mean", "var", "count"):
            assert HI.same_bits(out[tag], twin[tag]), (name, tag)
    assert HI.same_bits(want["cond_mean"]["cond_mean"], twin["cond_mean"])
    orders = H.orders(HI.VARIANTS)
    assert len({tuple(o) for o in orders.values()}) == 5
    for order in orders.values():
        HI.assert_same(history_run(case, order, hist), order, want)
    for v in HI.VARIANTS:
        HI.assert_same(history_run(case, [v, v], hist), [v, v], want)
    HI.assert_same(history_run(case, HI.VARIANTS, hist, between=HI.refused), HI.VARIANTS, want)


@pytest.mark.parametrize("grid,C_,k", [((33, 33, 5), 1, 3), ((17, 17, 9), 1, 0), ((9, 9, 5), 8, 0)], ids=gid)
def test_stream_contract(grid, C_, k):
    """tests/test_gpu_rbstats.py::test_stream_contract on a DMDA handle: a fresh handle whose first device call is on a side stream
    gives the bits of a twin on the default stream; a reset followed by updates on another stream gives them again; and update,
    cond_mean and get_fields return while the stream is still busy with a slow producer queued before them"""
    import torch

    n, T = int(np.prod(grid)), 3
    lr = R.lowrank(n, k, seed=1)
    b = R.rhs(n, seed=1)
    steps = [dev(R.samples(n, C_, seed=s)) for s in range(T)]
    a = torch.randn((4096, 4096), dtype=torch.float64, device="cuda") / 64.0
    scratch = torch.empty_like(a)
    torch.mm(a, a, out=scratch)
    torch.cuda.synchronize()

    def run(rb, inputs=steps):
        for Y in inputs:
            rb.update(Y)
        return rb.fields() + (rb.cond_mean(inputs[0]),)

    side_h, twin_h, warm = (handles(grid, C_, lr, b)[0] for _ in range(3))
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        side = run(side_h)
    st.synchronize()
    twin = run(twin_h)
    torch.cuda.synchronize()
    for s, t in zip(side, twin):
        same(s, t)
    twin_h.reset()  # reset, then the same updates on another stream
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        again = run(twin_h)
    other.synchronize()
    for s, t in zip(again, twin):
        same(s, t)
    run(warm)
    warm.reset()
    torch.cuda.synchronize()
    Yp = [torch.full_like(Y, float("nan")) for Y in steps]
    busy = torch.cuda.Event()
    with torch.cuda.stream(st):
        for _ in range(24):
            torch.mm(a, a, out=scratch)
        busy.record()
        for p, Y in zip(Yp, steps):
            p.copy_(Y, non_blocking=True)
        got = run(warm, Yp)
        returned_early = not busy.query()
    st.synchronize()
    assert returned_early, "the calls returned after the producer had finished: they synchronise the host, or the delay is too short"
    for s, t in zip(got, twin):
        same(s, t)
