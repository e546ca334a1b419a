"""The coloured block Gibbs sampler on the device (pmg_blockgibbs, kernels_blockgibbs.hip) against tests/blockgibbs_cases.py.

  apply, sweep_xi            bit-equal to the walk-through (the kernel's order of operations with the library's own W), forward,
                             backward and symmetric, on every width class, partial wavefronts, empty exteriors, rows in no
                             block and a layout with ld > n
  walk-through               within the reference's own bound of the plain numpy reference (ref_sweep's docstring)
  get_block_factor           W against inv(cholesky(A_PP)) by fwd_bound(m, kappa) of tests/chol_edge_refs.py
  sample                     against sweep_xi fed the oracle's slot normals, by noise_bound with NORMAL_TOL
  the stationary covariance  of the maps measured on the device is A^-1 to 1e-10
"""
import numpy as np
import pytest

import oracle as O
from blockgibbs_cases import (BWD, FWD, SYM, Reference, banded, cell_blocks, colors_valid, consecutive_blocks, covariance_error, directions, first_fit_colors, line_blocks, noise_bound, ref_apply, squared, star_blocks,
                              two_components, walk_apply)
from chol_edge_refs import fwd_bound
from woodbury_cases import NORMAL_TOL

pytestmark = pytest.mark.gpu
TYPES = (FWD, BWD, SYM)


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def make(A, blocks, colors=None, layout=None):
    from parmgmc_amd import BlockGibbs

    return BlockGibbs(A.rowptr, A.colidx, A.vals, blocks, block_colors=colors, layout=layout).setup()


def _grid_cases():
    e5, e05 = O.ex6_matrix(9, 0.5), O.ex6_matrix(9, 0.05)
    out = {}
    for name, A, pat in (("ex6sq", squared(e5), e5), ("ex6", e05, e05)):
        out[f"{name}-stars"] = (A, star_blocks(pat), None, None)
        out[f"{name}-cells"] = (A, cell_blocks(9, 9), None, None)
        out[f"{name}-lines"] = (A, line_blocks(9, 9), None, None)
    L3 = O.shifted_laplace(5, 4, 3, 2.0)
    out["lap3d-stars"] = (L3, star_blocks(L3), None, None)
    return out


SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)


def _banded_cases():
    A = banded(300, 70)
    # 310 rows of blocks on 300 rows: a block that would run past the end is moved up (the last two overlap); one colour each
    single, row = [], 0
    for m in SIZES:
        single += consecutive_blocks([m], min(row, 300 - m))
        row += m
    # mixed: three regions more than a half-bandwidth apart, one block of each in a colour, so that widths share a launch
    mixed, colors = [], []
    for c, trio in enumerate([(64, 63, 17), (33, 32, 16), (31, 15, 9), (8, 7, 5), (4, 3, 2), (1,)]):
        for m, start in zip(trio, (0, 135, 270)):
            mixed += consecutive_blocks([m], start)
            colors.append(c)
    assert sorted(len(p) for p in mixed) == sorted(SIZES)
    return {"banded-one-colour-each": (A, single, np.arange(16), None), "banded-mixed": (A, mixed, np.array(colors), None)}


def _edge_cases():
    out = {}
    # colours of 1, 7, 8 and 9 blocks of at most 8 rows on a tridiagonal matrix: blocks one gap row apart do not conflict; the
    # gap rows and the rows behind the last block are in no block
    T = banded(400, 1, seed=13)
    blocks, colors, row = [], [], 0
    for c, count in enumerate((1, 7, 8, 9)):
        for q in range(count):
            m = 1 + (3 * q + c) % 8
            blocks += consecutive_blocks([m], row)
            colors.append(c)
            row += m + 1
    out["partial-wavefronts"] = (T, blocks, np.array(colors), None)
    # a block that is a whole connected component: empty exterior (and a tile whose exterior width is zero)
    Cc = two_components(9, 40)
    out["component"] = (Cc, [np.arange(9)] + consecutive_blocks([2] * 10, 9), None, None)
    # vectors in a layout: a random placement with ld > n
    A = O.ex6_matrix(9, 0.05)
    pos = np.random.default_rng(5).permutation(81 + 37)[:81]
    out["layout"] = (A, star_blocks(A), None, (81 + 37, pos))
    return out


CASES = {**_grid_cases(), **_banded_cases(), **_edge_cases()}
_made = {}


def case(name):
    """(A, blocks, colours, pos, ld, handle, Ws, Reference), built once"""
    if name not in _made:
        A, blocks, colors, layout = CASES[name]
        bg = make(A, blocks, colors, layout)
        col = bg.get_coloring()
        if colors is None:
            assert np.array_equal(col, first_fit_colors(A, blocks))
        else:
            assert np.array_equal(col, colors)
        assert colors_valid(A, blocks, col) and bg.get_num_colors() == col.max() + 1 and bg.get_num_slots() == sum(len(p) for p in blocks)
        ld, pos = (A.n, np.arange(A.n)) if layout is None else layout
        _made[name] = (A, blocks, col, np.asarray(pos), ld, bg, [bg.block_factor(p) for p in range(len(blocks))], Reference(A, blocks))
    return _made[name]


def vectors(name, ld, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(ld), rng.standard_normal(ld)


@pytest.mark.parametrize("name", list(CASES))
def test_apply_and_sweep_xi_equal_the_walk_through_bit_for_bit(name):
    A, blocks, col, pos, ld, bg, Ws, R = case(name)
    b, y = vectors(name, ld, 1)
    xi = [np.random.default_rng(2 + d).standard_normal(bg.get_num_slots()) for d in range(2)]
    bd = dev(b)
    untouched = np.setdiff1d(np.arange(ld), pos[np.unique(np.concatenate(blocks))])
    for t in TYPES:
        bg.set_sweep_type(t)
        yd = dev(y)
        bg.apply(bd, yd)
        got, want = host(yd), walk_apply(A, blocks, col, Ws, b, y, t, None, pos)
        assert np.array_equal(got, want), (name, t, int((got != want).sum()))
        assert np.array_equal(got[untouched], y[untouched])  # rows in no block, layout padding
        yd = dev(y)
        for d, dr in enumerate(directions(t)):  # the same sample with injected normals, one directional sweep per call
            bg.sweep_xi(dev(xi[d]), bd, yd, backward=dr == BWD)
        got, want = host(yd), walk_apply(A, blocks, col, Ws, b, y, t, lambda d: xi[d], pos)
        assert np.array_equal(got, want), (name, t, int((got != want).sum()))
        assert np.array_equal(got[untouched], y[untouched])
    # negative control: the comparison sees one wrong bit
    want[pos[blocks[0][0]]] = np.nextafter(want[pos[blocks[0][0]]], np.inf)
    assert not np.array_equal(got, want)


@pytest.mark.parametrize("name", list(CASES))
def test_walk_through_is_within_the_reference_bound(name):
    A, blocks, col, pos, ld, bg, Ws, R = case(name)
    b, y = vectors(name, A.n, 3)
    xi = [np.random.default_rng(4 + d).standard_normal(bg.get_num_slots()) for d in range(2)]
    for t in TYPES:
        for xf in (None, lambda d: xi[d]):
            want, e = ref_apply(R, col, b, y, t, xf, bound=True)
            got = walk_apply(A, blocks, col, Ws, b, y, t, xf)
            ratio = float((np.abs(got - want) / np.maximum(e, 1e-300)).max())
            print(f"{name} type {t} noisy {xf is not None}: max |walk - ref| / bound = {ratio:.3g}")
            assert np.all(np.abs(got - want) <= e), (name, t, ratio)


@pytest.mark.parametrize("name", list(CASES))
def test_block_factors(name):
    A, blocks, col, pos, ld, bg, Ws, R = case(name)
    worst = 0.0
    for p, W in enumerate(Ws):
        K = R.blk[p]
        assert W.shape == K["W"].shape and np.array_equal(W, np.tril(W))
        err, bound = np.abs(W - K["W"]).max(), fwd_bound(len(blocks[p]), K["kappa"]) * np.abs(K["W"]).max()
        worst = max(worst, err / bound)
        assert err <= bound, (name, p, err, bound)
    print(f"{name}: max |W - inv(chol(A_PP))| / bound = {worst:.3g}")


@pytest.mark.parametrize("sweep", [FWD, SYM], ids=["forward", "symmetric"])
@pytest.mark.parametrize("name", ["ex6sq-stars", "banded-mixed", "layout"])
def test_sample_against_injected_oracle_normals(name, sweep):
    A, blocks, col, pos, ld, bg, Ws, R = case(name)
    ns, nd = bg.get_num_slots(), len(directions(sweep))
    b, y = vectors(name, ld, 6)
    bd = dev(b)
    bg.set_sweep_type(sweep)
    yd = dev(y)
    assert bg.sample(bd, yd, 3, seed=0xCAFE, counter0=5) == 5 + 3 * nd
    got = host(yd)

    scales = [0.0, 0.0]  # the largest iterate and the largest normal the fed chains meet

    def fed(counter0):
        yf, c = dev(y), counter0
        for _ in range(3):
            for dr in directions(sweep):
                xi = O.noise_rows(ns, 0xCAFE, c)
                bg.sweep_xi(dev(xi), bd, yf, backward=dr == BWD)
                scales[:] = max(scales[0], float(yf.abs().max())), max(scales[1], float(np.abs(xi).max()))
                c += 1
        return host(yf)

    want = fed(5)
    e = noise_bound(A, blocks, col, Ws, sweep, 3, NORMAL_TOL, max(scales[0], float(np.abs(y).max())), float(np.abs(b).max()), scales[1])
    diff = np.abs(got - want)[pos]
    print(f"{name} sweep {sweep}: max |sample - fed| = {diff.max():.3g}, max ratio to the bound {float((diff / np.maximum(e, 1e-300)).max()):.3g}")
    assert np.all(diff <= e)
    shifted = np.abs(got - fed(6))[pos]  # negative control: the counter shifted by one is another chain
    assert shifted.max() > 1e6 * e.max()


def test_stationary_covariance_of_the_device_maps():
    """the north star on the device: G from 81 apply calls, the noise map from nslots sweep_xi calls with unit xi and b = y = 0"""
    import torch

    A, blocks, col, pos, ld, bg, Ws, R = case("ex6sq-stars")
    n, ns = A.n, bg.get_num_slots()
    zero = torch.zeros(n, dtype=torch.float64, device="cuda")
    maps = {}
    for dr in (FWD, BWD):
        bg.set_sweep_type(dr)
        Y = torch.eye(n, dtype=torch.float64, device="cuda")
        for j in range(n):
            bg.apply(zero, Y[j])
        Xi, Nn = torch.eye(ns, dtype=torch.float64, device="cuda"), torch.zeros(ns, n, dtype=torch.float64, device="cuda")
        for s in range(ns):
            bg.sweep_xi(Xi[s], zero, Nn[s], backward=dr == BWD)
        maps[dr] = (host(Y).T, host(Nn).T)
    (Gf, Nf), (Gb, Nb) = maps[FWD], maps[BWD]
    ef, es = covariance_error(A, Gf, Nf), covariance_error(A, Gb @ Gf, np.hstack([Gb @ Nf, Nb]))
    print(f"covariance error of the device maps: forward {ef:.2e}, symmetric {es:.2e}")
    assert ef <= 1e-10 and es <= 1e-10


def test_errors():
    from parmgmc_amd import BlockGibbs, PMGError

    A = O.ex6_matrix(9, 0.05)
    stars = star_blocks(A)
    bad = first_fit_colors(A, stars)
    bad[1] = bad[0]  # stars 0 and 1 overlap
    with pytest.raises(PMGError) as e:
        make(A, stars, bad)
    assert e.value.code == 62 and "blocks 0 and 1" in str(e.value)
    B = banded(300, 70)
    with pytest.raises(PMGError) as e:
        BlockGibbs(B.rowptr, B.colidx, B.vals, [np.arange(65)])
    assert e.value.code == 56
    v = A.vals.copy()
    v[O.diag_pointers(A)[40]] = -1.0  # the centre of star 40
    with pytest.raises(PMGError) as e:
        BlockGibbs(A.rowptr, A.colidx, v, stars).setup()
    assert e.value.code == 81 and "block" in str(e.value)


def test_on_a_side_stream():
    """a fresh handle whose every device call is on a non-default stream gives the bits of a twin on the default stream"""
    import torch

    A, blocks, colors, layout = CASES["banded-mixed"]
    b, y = vectors("stream", A.n, 8)
    xi = np.random.default_rng(9).standard_normal(sum(len(p) for p in blocks))

    def script(bg):
        bd, out = dev(b), {}
        bg.set_sweep_type(SYM)
        out["apply"] = dev(y)
        bg.apply(bd, out["apply"])
        out["sample"] = dev(y)
        out["counter"] = bg.sample(bd, out["sample"], 2, seed=7, counter0=1)
        out["xi"] = dev(y)
        bg.sweep_xi(dev(xi), bd, out["xi"], backward=True)
        return out

    side_h, twin_h = make(A, blocks, colors), make(A, blocks, colors)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        side = script(side_h)
    st.synchronize()
    twin = script(twin_h)
    torch.cuda.synchronize()
    assert side["counter"] == twin["counter"] == 5
    for k in ("apply", "sample", "xi"):
        assert bool(torch.isfinite(side[k]).all()) and torch.equal(side[k], twin[k]), k
    assert not torch.equal(side["apply"], side["sample"])
