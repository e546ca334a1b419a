"""The call-history contract of the header for pmg_rbstats: what a call returns depends on the handle's construction, its current
settings and the call's arguments only, not on what was called before.  tests/test_gpu_call_history.py checks this for the
handles catalogued in tests/handle_steps.py; RBStats (parmgmc_amd/rbstats.py) is checked here in the same way: every step alone on
a handle of its own gives the reference bits, and the steps in five orders, each step twice, and the steps with a refused call
in between give those bits again, with the inputs left unchanged.  Every step starts with reset: the running sums are state by
design."""
import numpy as np
import pytest

import handle_steps as H
import oracle as O

pytestmark = pytest.mark.gpu
NCHAINS, NSTEPS = 8, 3
ARG_NULL, ARG_WRONG = 85, 62
CASES = ["ex6", "ex6_k3"]
VARIANTS = ["updates", "readouts_between", "reset_in_between", "cond_mean"]
ORDER_IDS = ["listed", "reversed"] + [f"perm{s}" for s in H.PERMUTATION_SEEDS]


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


@pytest.fixture(scope="module")
def ctx():
    """the ~1000-row ex6 operator, the inputs (made once, read only) and the reference bits per case"""
    A = O.ex6_matrix(32, 1e-2)
    rng = np.random.default_rng(8)
    x = {f"Y{i}": dev(rng.standard_normal((A.n, NCHAINS))) for i in range(NSTEPS)}
    return {"A": A, "x": x, "alone": {}}


def build(case, ctx):
    from parmgmc_amd import RBStats

    A = ctx["A"]
    rng = np.random.default_rng(10)
    lowrank = (rng.uniform(-1.0, 1.0, (A.n, 3)) / np.sqrt(A.n), np.array([2.0, 5.0, 11.0]))
    return RBStats(A, NCHAINS, lowrank=lowrank if case == "ex6_k3" else None, b=dev(rng.standard_normal(A.n)))


def readout(rb):
    mean, var = rb.fields()
    return {"mean": mean, "var": var, "count": rb.count()}


def step(variant, rb, x):
    rb.reset()
    out = {}
    if variant == "reset_in_between":  # other updates, forgotten
        rb.update(x["Y2"])
        rb.update(x["Y0"])
        readout(rb)
        rb.reset()
    if variant == "cond_mean":  # records nothing
        out["cond_mean"] = rb.cond_mean(x["Y1"])
    for i in range(NSTEPS):
        rb.update(x[f"Y{i}"])
        if variant == "readouts_between" and i:
            readout(rb)
            rb.cond_mean(x["Y2"])
    out.update(readout(rb))
    return out


def refused(i, rb, x):
    """a call the host refuses before any launch, with the status the header documents"""
    from parmgmc_amd.capi import lib
    from parmgmc_amd.wrappers import _ptr, _stream

    if i % 2:
        assert lib.pmg_rbstats_update(rb._h, None, _stream()) == ARG_NULL
    else:
        assert lib.pmg_rbstats_cond_mean(rb._h, _ptr(x["Y0"]), _ptr(x["Y0"]), _stream()) == ARG_WRONG


def same_bits(a, b):
    import torch

    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))
    return type(a) is type(b) and a == b


def run(case, order, ctx, between=None):
    """{position: results} of the steps of `order` on one new handle; after every step the inputs are what they were"""
    import torch

    rb, x = build(case, ctx), {k: v.clone() for k, v in ctx["x"].items()}
    out = []
    for i, name in enumerate(order):
        if between is not None and i:
            between(i, rb, x)
        out.append(step(name, rb, x))
        torch.cuda.synchronize()
        for k, v in ctx["x"].items():
            assert same_bits(x[k], v), f"step {name!r} left input {k!r} changed; call order: {order}"
    return out


def alone(case, ctx):
    if case not in ctx["alone"]:
        ctx["alone"][case] = {v: run(case, [v], ctx)[0] for v in VARIANTS}
    return ctx["alone"][case]


def assert_same(got, order, want):
    for res, name in zip(got, order):
        assert res.keys() == want[name].keys(), name
        for tag in res:
            assert same_bits(res[tag], want[name][tag]), f"step {name!r}, tag {tag!r} differs from the step on a handle of its own; call order: {order}"


@pytest.mark.parametrize("case", CASES)
def test_alone(case, ctx):
    """the read-outs, cond_mean and a reset in between leave the fields of the three updates unchanged"""
    import torch

    res = alone(case, ctx)
    for name, out in res.items():
        assert out["count"] == (NSTEPS, NSTEPS * NCHAINS)
        for tag, v in out.items():
            if isinstance(v, torch.Tensor):
                assert bool(torch.isfinite(v).all()), (name, tag)
        for tag in res["updates"]:
            assert same_bits(out[tag], res["updates"][tag]), (name, tag)
    assert res["cond_mean"]["cond_mean"].shape == (ctx["A"].n, NCHAINS)


@pytest.mark.parametrize("order_id", ORDER_IDS)
@pytest.mark.parametrize("case", CASES)
def test_orders(case, order_id, ctx):
    orders = H.orders(VARIANTS)
    assert len({tuple(o) for o in orders.values()}) == len(ORDER_IDS)
    order = orders[order_id]
    assert_same(run(case, order, ctx), order, alone(case, ctx))


@pytest.mark.parametrize("case", CASES)
def test_twice(case, ctx):
    for v in VARIANTS:
        assert_same(run(case, [v, v], ctx), [v, v], alone(case, ctx))


@pytest.mark.parametrize("case", CASES)
def test_a_refused_call_in_between(case, ctx):
    assert_same(run(case, VARIANTS, ctx, between=refused), VARIANTS, alone(case, ctx))


def test_control_a_step_without_reset_fails_the_comparison(ctx):
    """a step that does not start with reset depends on what came before: the comparison sees it"""
    rb, x = build("ex6", ctx), ctx["x"]
    step("updates", rb, x)
    for i in range(NSTEPS):
        rb.update(x[f"Y{i}"])
    later = readout(rb)
    want = alone("ex6", ctx)["updates"]
    assert later["count"] == (2 * NSTEPS, 2 * NSTEPS * NCHAINS)
    assert same_bits(later["mean"], want["mean"]) is False or same_bits(later["var"], want["var"]) is False
