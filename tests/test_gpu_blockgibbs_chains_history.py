"""The call-history and stream contracts of include/parmgmc_hip.h for the chains entry points of the coloured block Gibbs handle
(pmg_blockgibbs_*_chains): the only per-object state is the device copy of the seeds, and it never shows.  The steps go through
the machinery of tests/test_gpu_call_history.py and tests/handle_steps.py, as tests/test_gpu_blockgibbs_history.py does for the
single-chain calls, on the same 81-row star handle: every step alone on a handle of its own, all of them on one handle in five
orders, each twice in a row, and with a call the host refuses before any launch between every two steps.  The steps grow the
key buffer (3 -> 65 chains), replace the seeds at the same size, and mix in the single-chain sample.

Streams (helpers of tests/test_gpu_stream_contract.py): a chains call on a side stream behind a slow producer returns before its
input exists and gives the default-stream result; a captured call replays on new data (its seeds were uploaded by the identical
warm call, so nothing synchronises during capture)."""
import numpy as np
import pytest

import handle_steps as H
import test_gpu_blockgibbs_history as BH
import test_gpu_call_history as CH
import test_gpu_stream_contract as SC
from handle_steps import ARG_NULL, ARG_OUTOFRANGE, Failing, Step, Subject, status
from test_gpu_stream_contract import delay, streams  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ORDER_IDS = ["listed", "reversed"] + [f"perm{s}" for s in H.PERMUTATION_SEEDS]
SEEDS_A, SEEDS_C = [11, 12, 13], [0x9E3779B97F4A7C15, 12, 2**64 - 1]
SEEDS_B = [1000 + 3 * c for c in range(65)]


def inputs():
    rng = np.random.default_rng(4)
    x = {"b": rng.standard_normal(81), "y": rng.standard_normal(81), "Y3": rng.standard_normal((81, 3)), "Y65": rng.standard_normal((81, 65)), "B3": rng.standard_normal((81, 3)),
         "Xi3": rng.standard_normal((369, 3))}
    return SC.to_dev(x)


def _ch(tag, start, call, sweep_type=None):
    """a step: call(bg, x, Y) on a fresh copy Y of x[start], under sweep type `sweep_type` (set, call, set back)"""
    def fn(bg, x):
        Y, t0 = x[start].clone(), bg.get_sweep_type()
        if sweep_type is not None:
            bg.set_sweep_type(sweep_type)
        out = {tag: Y, tag + "_counter": call(bg, x, Y) or 0}
        bg.set_sweep_type(t0)
        return out

    return fn


def steps():
    return [Step("apply_chains", _ch("apply_chains", "Y3", lambda bg, x, Y: bg.apply_chains(x["b"], Y)), ["b"], ["BlockGibbs.apply_chains"]),
            Step("sample_chains_A", _ch("sample_chains_A", "Y3", lambda bg, x, Y: bg.sample_chains(x["b"], Y, 2, SEEDS_A, counter0=3)), ["b"], ["BlockGibbs.sample_chains"]),
            Step("sample_chains_B65", _ch("sample_chains_B65", "Y65", lambda bg, x, Y: bg.sample_chains(x["b"], Y, 1, SEEDS_B, counter0=7), 3), ["b"], ["BlockGibbs.sample_chains"]),
            Step("sample_chains_C", _ch("sample_chains_C", "Y3", lambda bg, x, Y: bg.sample_chains(x["b"], Y, 2, SEEDS_C, counter0=3)), ["b"], ["BlockGibbs.sample_chains"]),
            Step("sample_chains_rhs", _ch("sample_chains_rhs", "Y3", lambda bg, x, Y: bg.sample_chains(x["B3"], Y, 1, SEEDS_A, counter0=9), 2), ["B3"], ["BlockGibbs.sample_chains"]),
            Step("sweep_xi_chains", _ch("sweep_xi_chains", "Y3", lambda bg, x, Y: bg.sweep_xi_chains(x["Xi3"], x["b"], Y)), ["b", "Xi3"], ["BlockGibbs.sweep_xi_chains"]),
            Step("sample", _ch("sample", "y", lambda bg, x, y: bg.sample(x["b"], y, 2, seed=5, counter0=3)), ["b"], ["BlockGibbs.sample"])]


def failing():
    from parmgmc_amd.capi import lib
    from parmgmc_amd.wrappers import _ptr, _stream

    def null_seeds(bg, x):
        import ctypes as C

        out = C.c_uint64()
        return lib.pmg_blockgibbs_sample_chains(bg._h, 3, None, _ptr(x["b"]), _ptr(x["Y3"].clone()), 1, 0, C.byref(out), None, None, _stream())

    return [Failing("nchains_zero", lambda bg, x: lib.pmg_blockgibbs_apply_chains(bg._h, 0, _ptr(x["b"]), _ptr(x["Y3"].clone()), _stream()), ARG_OUTOFRANGE),
            Failing("null_seeds", null_seeds, ARG_NULL),
            Failing("its_negative", lambda bg, x: status(lambda: bg.sample_chains(x["b"], x["Y3"].clone(), -1, SEEDS_C)), ARG_OUTOFRANGE),
            Failing("null_xi", lambda bg, x: lib.pmg_blockgibbs_sweep_xi_chains(bg._h, 3, 0, None, _ptr(x["b"]), _ptr(x["Y3"].clone()), _stream()), ARG_NULL)]


@pytest.fixture(scope="module")
def ctx():
    return {"alone": {}, "inputs": {}}


@pytest.fixture(scope="module")
def sub():
    return Subject("blockgibbs_chains", "ex6_stars", BH.build, inputs, steps(), failing())


def test_alone(sub, ctx):
    import torch

    res = CH.alone(sub, ctx)
    assert res.keys() == {s.name for s in sub.steps}
    for name, out in res.items():
        assert bool(torch.isfinite(out[name]).all()), name
    assert res["sample_chains_A"]["sample_chains_A_counter"] == 5 and res["sample_chains_B65"]["sample_chains_B65_counter"] == 9
    assert res["sample_chains_rhs"]["sample_chains_rhs_counter"] == 10 and res["sample"]["sample_counter"] == 5
    flat = [SC.host(res[s.name][s.name]).tobytes() for s in sub.steps]
    assert len(set(flat)) == len(flat)  # seven different results: a mix-up would show
    # A and C share the seed of chain 1 only
    a, c = res["sample_chains_A"]["sample_chains_A"], res["sample_chains_C"]["sample_chains_C"]
    assert torch.equal(a[:, 1], c[:, 1]) and not torch.equal(a[:, 0], c[:, 0]) and not torch.equal(a[:, 2], c[:, 2])


@pytest.mark.parametrize("order_id", ORDER_IDS)
def test_orders(sub, ctx, order_id):
    names = [s.name for s in sub.steps]
    orders = H.orders(names)
    assert len({tuple(o) for o in orders.values()}) == 5
    CH.assert_same_results(CH.run(sub, orders[order_id], ctx), CH.alone(sub, ctx), orders[order_id])


def test_twice(sub, ctx):
    want = CH.alone(sub, ctx)
    for s in sub.steps:
        again = Step(s.name + "_again", s.fn, s.const, s.calls)
        got = CH.run(sub, [s.name, again.name], ctx, extra={again.name: again})
        CH.assert_same_results({s.name: got[s.name]}, want, [s.name])
        CH.assert_same_results({s.name: got[again.name]}, want, [s.name])


def test_a_failing_call_in_between(sub, ctx):
    order = [s.name for s in sub.steps]
    made = []

    def between(i, handle, x):
        f = sub.failing[(i - 1) % len(sub.failing)]
        st = f.fn(handle, x)
        made.append(f.name)
        assert st == f.status, f"{f.name}: status {st}, documented {f.status}"

    CH.assert_same_results(CH.run(sub, order, ctx, between=between), CH.alone(sub, ctx), order)
    assert set(made) == {f.name for f in sub.failing}


def test_control_seeds_left_from_the_call_before_would_fail_the_comparison(sub, ctx):
    """what a stale key buffer would give: seeds A in the place of seeds C is seen as a difference of that step"""
    want = CH.alone(sub, ctx)
    stale = Step("sample_chains_C", _ch("sample_chains_C", "Y3", lambda bg, x, Y: bg.sample_chains(x["b"], Y, 2, SEEDS_A, counter0=3)), ["b"], ["BlockGibbs.sample_chains"])
    order = ["sample_chains_A", "sample_chains_C"]
    got = CH.run(sub, order, ctx, extra={stale.name: stale})
    assert CH.first_difference(got, want, order) == ("sample_chains_C", "sample_chains_C")


NC = 8


def _steady(rhs):
    bg = BH.build()
    seeds = list(range(31, 31 + NC))
    return (lambda b, Y: bg.sample_chains(b, Y, 2, seeds, counter0=3)), ((81, NC) if rhs else (81,)), (81, NC)


@pytest.mark.parametrize("rhs", [False, True], ids=["shared_b", "per_chain_b"])
def test_ordered_behind_a_slow_producer(rhs, delay, streams):  # noqa: F811
    """tests/test_gpu_stream_contract.py::test_ordered_behind_a_slow_producer for a chains call: on a side stream whose inputs are
    still poison when the call returns, the result is the default-stream result"""
    import torch

    call, bshape, yshape = _steady(rhs)
    b, y0 = SC.steady_inputs(bshape, yshape, 21)
    want = y0.clone()
    call(b, want)  # the default-stream result; the seeds are uploaded from here on
    torch.cuda.synchronize()
    st, third = streams
    b_side, y_side = torch.full_like(b, float("nan")), torch.full_like(y0, float("nan"))
    torch.cuda.synchronize()
    with SC.no_collection(), torch.cuda.stream(st):
        delay()
        b_side.copy_(b)
        y_side.copy_(y0)
        with torch.cuda.stream(third):
            seen_queued = b_side.clone()
        call(b_side, y_side)
        with torch.cuda.stream(third):
            seen_returned = b_side.clone()
    torch.cuda.synchronize()
    assert bool(torch.isnan(seen_queued).all()), "delay too short: the poison was gone once the producer was queued"
    assert bool(torch.isnan(seen_returned).all()), "delay too short: the poison was gone when the call returned (or the call synchronises the host)"
    assert torch.equal(b_side, b)
    assert torch.equal(y_side, want)
    assert not torch.equal(want, y0)


def test_capture_and_replay():
    """the body of tests/test_gpu_stream_contract.py::test_capture_and_replay applies to a chains call unchanged: the warm call on
    the capture stream uploads the seeds, the captured call finds them and synchronises nothing"""
    import torch

    call, bshape, yshape = _steady(False)
    b_static, y_static = SC.steady_inputs(bshape, yshape, 22)
    b_new, y_new = SC.steady_inputs(bshape, yshape, 23)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        call(b_static, y_static)  # warm on the capture stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        call(b_static, y_static)
    b_static.copy_(b_new)
    y_static.copy_(y_new)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want = y_new.clone()
    call(b_new, want)
    torch.cuda.synchronize()
    assert torch.equal(b_static, b_new)
    assert torch.equal(y_static, want)
    assert not torch.equal(want, y_new)
