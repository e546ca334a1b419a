"""The call-history contract of include/parmgmc_hip.h for the coloured block Gibbs handle: a call's results depend on the
object's construction, its current settings and the call's arguments only, not on what was called before.  The steps of
parmgmc_amd.BlockGibbs (apply, sample, sweep_xi under the three sweep types) go through the machinery of
tests/test_gpu_call_history.py (run / alone / assert_same_results) and the orders of tests/handle_steps.py: every step alone
on a handle of its own, then all of them on one handle in five orders, each twice in a row, and with a call the host
refuses before any launch between every two steps."""
import numpy as np
import pytest

import handle_steps as H
import oracle as O
import test_gpu_call_history as CH
import test_gpu_stream_contract as SC
from handle_steps import ARG_NULL, ARG_OUTOFRANGE, ARG_WRONGSTATE, SUP, Failing, Step, Subject, status

pytestmark = pytest.mark.gpu
ORDER_IDS = ["listed", "reversed"] + [f"perm{s}" for s in H.PERMUTATION_SEEDS]


def build():
    """vertex-star blocks (overlapping, 3 to 5 rows, 369 slots) on the ex6 operator of a 9 x 9 grid"""
    from parmgmc_amd import BlockGibbs

    A = O.ex6_matrix(9, 0.05)
    return BlockGibbs(A.rowptr, A.colidx, A.vals, (A.rowptr, A.colidx)).setup()


def inputs():
    rng = np.random.default_rng(4)
    return SC.to_dev({"b": rng.standard_normal(81), "y": rng.standard_normal(81), "xi": rng.standard_normal(369)})


def _bg(tag, call, sweep_type=None):
    """a step: call(bg, x, y) on a fresh copy y of the iterate, under sweep type `sweep_type` (set, call, set back)"""
    def fn(bg, x):
        y, t0 = x["y"].clone(), bg.get_sweep_type()
        if sweep_type is not None:
            bg.set_sweep_type(sweep_type)
        out = {tag: y, tag + "_counter": call(bg, x, y) or 0}
        bg.set_sweep_type(t0)
        return out

    return fn


def steps():
    return [Step("apply", _bg("apply", lambda bg, x, y: bg.apply(x["b"], y)), ["b"], ["BlockGibbs.apply"]),
            Step("apply_symmetric", _bg("apply_symmetric", lambda bg, x, y: bg.apply(x["b"], y), 3), ["b"], ["BlockGibbs.apply"]),
            Step("sample", _bg("sample", lambda bg, x, y: bg.sample(x["b"], y, 2, seed=5, counter0=3)), ["b"], ["BlockGibbs.sample"]),
            Step("sample_backward", _bg("sample_backward", lambda bg, x, y: bg.sample(x["b"], y, 1, seed=6, counter0=9), 2), ["b"], ["BlockGibbs.sample"]),
            Step("sweep_xi", _bg("sweep_xi", lambda bg, x, y: bg.sweep_xi(x["xi"], x["b"], y)), ["b", "xi"], ["BlockGibbs.sweep_xi"]),
            Step("sweep_xi_backward", _bg("sweep_xi_backward", lambda bg, x, y: bg.sweep_xi(x["xi"], x["b"], y, backward=True)), ["b", "xi"], ["BlockGibbs.sweep_xi"])]


def failing():
    from parmgmc_amd.capi import lib
    from parmgmc_amd.wrappers import _ptr, _stream

    return [Failing("null_b", lambda bg, x: lib.pmg_blockgibbs_apply(bg._h, None, _ptr(x["y"].clone()), _stream()), ARG_NULL),
            Failing("its_negative", lambda bg, x: status(lambda: bg.sample(x["b"], x["y"].clone(), -1, seed=1)), ARG_OUTOFRANGE),
            Failing("null_xi", lambda bg, x: lib.pmg_blockgibbs_sweep_xi(bg._h, 0, None, _ptr(x["b"]), _ptr(x["y"].clone()), _stream()), ARG_NULL),
            Failing("sweep_type", lambda bg, x: status(lambda: bg.set_sweep_type(4)), SUP),
            Failing("coloring_after_setup", lambda bg, x: lib.pmg_blockgibbs_set_coloring(bg._h, 0, None), ARG_WRONGSTATE)]


@pytest.fixture(scope="module")
def ctx():
    return {"alone": {}, "inputs": {}}


@pytest.fixture(scope="module")
def sub():
    return Subject("blockgibbs", "ex6_stars", build, inputs, steps(), failing())


def test_alone(sub, ctx):
    import torch

    res = CH.alone(sub, ctx)
    assert res.keys() == {s.name for s in sub.steps}
    for name, out in res.items():
        assert bool(torch.isfinite(out[name]).all()), name
    assert res["sample"]["sample_counter"] == 5 and res["sample_backward"]["sample_backward_counter"] == 10
    # the steps are six different results: a comparison of them with each other would see a mix-up
    flat = [SC.host(res[s.name][s.name]).tobytes() for s in sub.steps]
    assert len(set(flat)) == len(flat)


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


def test_control_a_setting_left_changed_fails_the_comparison(sub, ctx):
    want = CH.alone(sub, ctx)
    leak = Step("leak", lambda bg, x: bg.set_sweep_type(2) or {"leak": 0}, [], ["BlockGibbs.set_sweep_type"])
    order = ["leak", "apply"]
    got = CH.run(sub, order, ctx, extra={leak.name: leak})
    assert CH.first_difference(got, want, order) == ("apply", "apply")
