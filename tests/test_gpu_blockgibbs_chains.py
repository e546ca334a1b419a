"""Many chains per launch of the coloured block Gibbs sampler (pmg_blockgibbs_*_chains, kernels_blockgibbs_chains.hip) against
the single-chain calls of the same handle, which tests/test_gpu_blockgibbs.py pins to the walk-through and the oracle.  Every
comparison is bit for bit (torch.equal / the int64 view); there is no tolerance anywhere in this module.

  bit identity      column c of apply_chains, sample_chains (shared b and one b per chain) and sweep_xi_chains equals apply / sample /
                    sweep_xi on that column alone, and the counters agree: every case x every C, the sweep type rotating over the
                    product so that every case and every C meets forward, backward and symmetric
  untouched memory  sentinels around Y, rows in no block and unused layout positions, at odd and tail-chunk C, on vectors that
                    are 8-byte and 16-byte aligned
  seeds             equal seeds and starts stay equal, different seeds differ; its = 2 is two calls of its = 1 chained by counter_out
  consumers         stats= and rb= together against handles updated by hand; a callback's non-zero return aborts with that status
  byte model        C = 1 is the single-chain model; affine in C with the documented slope

The kernel carries chunks of CB = 8 chains: C runs over 7, 8, 9 (the first chunk boundary), 16 and 17 (the second) besides the
small, odd and large counts."""
import numpy as np
import pytest

import test_gpu_blockgibbs as BG
from blockgibbs_cases import BWD, FWD, SYM

pytestmark = pytest.mark.gpu
NAMES = ["banded-mixed", "banded-one-colour-each", "partial-wavefronts", "component", "layout", "ex6sq-stars", "lap3d-stars"]
CB = 8
CS = sorted({1, 2, 3, 8, 9, 32, 33, 65, CB - 1, CB, CB + 1, 2 * CB, 2 * CB + 1})
TYPES = (FWD, BWD, SYM)
GOLDEN = 0x9E3779B97F4A7C15


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def bits(t):
    import torch

    return t.contiguous().view(torch.int64)


def _inputs(ld, nslots, C, seed):
    rng = np.random.default_rng(seed)
    return dev(rng.standard_normal(ld)), dev(rng.standard_normal((ld, C))), dev(rng.standard_normal((ld, C))), dev(rng.standard_normal((max(nslots, 1), C)))


def _columns(C, call, Y0):
    """the single-chain call on every column alone: (the columns stacked, the returned values)"""
    import torch

    cols, rets = [], []
    for c in range(C):
        y = Y0[:, c].clone()
        rets.append(call(c, y))
        cols.append(y)
    return torch.stack(cols, dim=1), rets


@pytest.mark.parametrize("name", NAMES)
def test_every_column_equals_the_single_chain_call(name):
    import torch

    A, blocks, col, pos, ld, bg, Ws, R = BG.case(name)
    ns = bg.get_num_slots()
    golden = name == "ex6sq-stars"  # one case on full 64-bit seeds and a counter beyond 2^32
    counter0 = 2**32 + 5 if golden else 3
    seen = set()
    try:
        for k, C in enumerate(CS):
            t = TYPES[(NAMES.index(name) + k) % 3]
            seen.add(t)
            bg.set_sweep_type(t)
            b, B, Y0, Xi = _inputs(ld, ns, C, 100 + C)
            seeds = [(GOLDEN + c) & (2**64 - 1) if golden else 1000 + 7 * c for c in range(C)]
            # apply
            Y = Y0.clone()
            bg.apply_chains(b, Y)
            want, _ = _columns(C, lambda c, y: bg.apply(b, y), Y0)
            assert torch.equal(bits(Y), bits(want)), (name, C, t, "apply")
            assert not torch.equal(Y, Y0)
            # sample, shared b
            Y = Y0.clone()
            ctr = bg.sample_chains(b, Y, 2, seeds, counter0=counter0)
            want, ctrs = _columns(C, lambda c, y: bg.sample(b, y, 2, seed=seeds[c], counter0=counter0), Y0)
            assert torch.equal(bits(Y), bits(want)), (name, C, t, "sample")
            assert set(ctrs) == {ctr} and ctr == counter0 + 2 * (2 if t == SYM else 1)
            # sample, one b per chain
            Y = Y0.clone()
            ctr = bg.sample_chains(B, Y, 2, seeds, counter0=counter0)
            want, ctrs = _columns(C, lambda c, y: bg.sample(B[:, c].contiguous(), y, 2, seed=seeds[c], counter0=counter0), Y0)
            assert torch.equal(bits(Y), bits(want)), (name, C, t, "sample_rhs")
            assert set(ctrs) == {ctr}
            if C > 1:
                assert not torch.equal(B[:, 0], B[:, 1])
            # injected normals, one directional sweep
            for backward in (False, True):
                Y = Y0.clone()
                bg.sweep_xi_chains(Xi, b, Y, backward=backward)
                want, _ = _columns(C, lambda c, y: bg.sweep_xi(Xi[:, c].contiguous(), b, y, backward=backward), Y0)
                assert torch.equal(bits(Y), bits(want)), (name, C, t, "sweep_xi", backward)
    finally:
        bg.set_sweep_type(FWD)
    assert seen == set(TYPES)


def test_control_the_comparison_sees_a_wrong_seed():
    import torch

    A, blocks, col, pos, ld, bg, Ws, R = BG.case("lap3d-stars")
    b, B, Y0, Xi = _inputs(ld, bg.get_num_slots(), 3, 5)
    Y = Y0.clone()
    bg.sample_chains(b, Y, 1, [1, 2, 3])
    want, _ = _columns(3, lambda c, y: bg.sample(b, y, 1, seed=[1, 2, 4][c]), Y0)
    assert torch.equal(bits(Y[:, :2]), bits(want[:, :2])) and not torch.equal(Y[:, 2], want[:, 2])


@pytest.mark.parametrize("name", ["partial-wavefronts", "layout"])
@pytest.mark.parametrize("C,lead", [(3, 5), (9, 5), (12, 5), (12, 4), (17, 3), (33, 1)])
def test_nothing_else_is_written(name, C, lead):
    """Y inside a larger buffer, `lead` doubles from its 16-byte aligned start: sentinels in front and behind, a second pattern
    on the rows in no block and the unused layout positions (finite: such rows are read as exterior columns)"""
    import torch

    A, blocks, col, pos, ld, bg, Ws, R = BG.case(name)
    rng = np.random.default_rng(7)
    tail = 64
    buf = torch.full((lead + ld * C + tail,), -1.5e300, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    Y = buf[lead : lead + ld * C].view(ld, C)
    assert Y.is_contiguous() and Y.data_ptr() % 16 == (8 if lead % 2 else 0)
    Y.copy_(dev(rng.standard_normal((ld, C))))
    touched = np.zeros(ld, bool)
    touched[pos[np.unique(np.concatenate(blocks))]] = True
    rest = torch.as_tensor(np.flatnonzero(~touched), device="cuda")
    assert len(rest) > 0
    Y[rest] = dev(3.0e5 + np.arange(len(rest) * C).reshape(len(rest), C))
    before = buf.clone()
    b, B = dev(rng.standard_normal(ld)), dev(rng.standard_normal((ld, C)))
    Xi = dev(rng.standard_normal((bg.get_num_slots(), C)))
    seeds = list(range(40, 40 + C))
    for t in TYPES:
        bg.set_sweep_type(t)
        bg.apply_chains(b, Y)
        bg.sample_chains(b, Y, 2, seeds)
        bg.sample_chains(B, Y, 1, seeds)
        bg.sweep_xi_chains(Xi, b, Y, backward=t == BWD)
    bg.set_sweep_type(FWD)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf[:lead]), bits(before[:lead]))
    assert torch.equal(bits(buf[lead + ld * C :]), bits(before[lead + ld * C :]))
    assert torch.equal(bits(Y[rest]), bits(before[lead : lead + ld * C].view(ld, C)[rest]))
    live = torch.as_tensor(np.flatnonzero(touched), device="cuda")
    assert bool((Y[live] != before[lead : lead + ld * C].view(ld, C)[live]).all())  # every row of a block in every column was written
    assert bool(torch.isfinite(Y).all())


def test_seeds_and_counters():
    import torch

    A, blocks, col, pos, ld, bg, Ws, R = BG.case("ex6sq-stars")
    rng = np.random.default_rng(11)
    b = dev(rng.standard_normal(ld))
    start = rng.standard_normal(ld)
    C = 9
    Y0 = dev(np.repeat(start[:, None], C, axis=1))
    seeds = [5, 6, 5, 7, 8, 9, 6, 10, 5]
    Y = Y0.clone()
    ctr = bg.sample_chains(b, Y, 2, seeds, counter0=3)
    assert ctr == 5
    for i in range(C):
        for j in range(i + 1, C):
            assert torch.equal(Y[:, i], Y[:, j]) == (seeds[i] == seeds[j]), (i, j)
    Z = Y0.clone()
    c1 = bg.sample_chains(b, Z, 1, seeds, counter0=3)
    c2 = bg.sample_chains(b, Z, 1, seeds, counter0=c1)
    assert (c1, c2) == (4, 5) and torch.equal(bits(Z), bits(Y))
    bg.set_sweep_type(SYM)
    try:
        Y = Y0.clone()
        assert bg.sample_chains(b, Y, 2, seeds, counter0=3) == 7
        Z = Y0.clone()
        c1 = bg.sample_chains(b, Z, 1, seeds, counter0=3)
        assert c1 == 5 and bg.sample_chains(b, Z, 1, seeds, counter0=c1) == 7
        assert torch.equal(bits(Z), bits(Y))
        Z = Y0.clone()
        assert bg.sample_chains(b, Z, 0, seeds, counter0=3) == 3 and torch.equal(bits(Z), bits(Y0))  # its = 0: nothing
    finally:
        bg.set_sweep_type(FWD)


def test_consumers_and_callback():
    import torch

    from parmgmc_amd import ChainStats, PMGError, RBStats

    A, blocks, col, pos, ld, bg, Ws, R = BG.case("ex6sq-stars")
    rng = np.random.default_rng(12)
    C, its = 8, 5
    b, Y0 = dev(rng.standard_normal(ld)), dev(rng.standard_normal((ld, C)))
    seeds = list(range(70, 70 + C))

    def fresh():
        return ChainStats(ld, C), RBStats(A, C, b=b)

    # by hand: five calls of its = 1, both handles updated after each
    cs0, rb0 = fresh()
    Y, ctr, steps = Y0.clone(), 2, []
    for _ in range(its):
        ctr = bg.sample_chains(b, Y, 1, seeds, counter0=ctr)
        cs0.update(Y), rb0.update(Y)
        steps.append(Y.clone())
    want = [f.clone() for f in cs0.fields() + rb0.fields()]
    # both consumers in one call
    cs, rb = fresh()
    Z = Y0.clone()
    assert bg.sample_chains(b, Z, its, seeds, counter0=2, stats=cs, rb=rb) == ctr
    assert torch.equal(bits(Z), bits(Y))
    assert cs.count() == cs0.count() == (its, its * C) and rb.count() == rb0.count()
    for got, w in zip(cs.fields() + rb.fields(), want):
        assert torch.equal(bits(got), bits(w))
    # each consumer alone goes through the library's own callback
    cs, rb = fresh()
    bg.sample_chains(b, Y0.clone(), its, seeds, counter0=2, stats=cs)
    bg.sample_chains(b, Y0.clone(), its, seeds, counter0=2, rb=rb)
    for got, w in zip(cs.fields() + rb.fields(), want):
        assert torch.equal(bits(got), bits(w))
    with pytest.raises(ValueError):
        bg.sample_chains(b, Y0.clone(), 1, seeds, stats=cs, callback=lambda it, Y: 0)
    # a callback that returns non-zero at step 2 aborts with that status; Y holds the step-2 sample
    calls = []

    def stop_at_2(it, Yt):
        calls.append(it)
        assert Yt is Z
        return 91 if it == 2 else 0

    Z = Y0.clone()
    with pytest.raises(PMGError) as e:
        bg.sample_chains(b, Z, its, seeds, counter0=2, callback=stop_at_2)
    assert e.value.code == 91 and calls == [0, 1, 2]
    torch.cuda.synchronize()
    assert torch.equal(bits(Z), bits(steps[2]))
    # under the symmetric sweep a sample is two directional sweeps: the callback sees whole samples only
    bg.set_sweep_type(SYM)
    try:
        seen = []
        Z = Y0.clone()
        bg.sample_chains(b, Z, 3, seeds, callback=lambda it, Yt: seen.append((it, Yt.clone())) and None)
        W = Y0.clone()
        c = 0
        for it in range(3):
            c = bg.sample_chains(b, W, 1, seeds, counter0=c)
            assert seen[it][0] == it and torch.equal(bits(seen[it][1]), bits(W))
        assert len(seen) == 3
    finally:
        bg.set_sweep_type(FWD)


@pytest.mark.parametrize("name", ["ex6sq-stars", "banded-mixed", "component"])
def test_byte_model(name):
    A, blocks, col, pos, ld, bg, Ws, R = BG.case(name)
    ns = bg.get_num_slots()
    one, two = bg.algorithmic_bytes_chains(1), bg.algorithmic_bytes_chains(2)
    assert one == bg.algorithmic_bytes()
    assert two - one == 16 * ns  # y read and written per chain; everything else is shared
    assert bg.algorithmic_bytes_chains(32) == one + 31 * (two - one) == one + 31 * 16 * ns
    r1, r2 = bg.algorithmic_bytes_chains(1, per_chain_rhs=True), bg.algorithmic_bytes_chains(2, per_chain_rhs=True)
    assert r1 == one and r2 - r1 == 24 * ns
    assert bg.algorithmic_bytes_chains(32, per_chain_rhs=True) == one + 31 * 24 * ns
