"""The contract of include/parmgmc_hip.h that a call's results depend on the object's construction, its current settings and the
call's arguments only: every step of tests/handle_steps.py gives, in any call order on one handle, the bits it gives on a handle of
its own.  Every comparison is bit for bit (the int64 view of the float64 tensors, so that -0.0 and NaN count) or == on returned
counters; no tolerance is involved in any comparison between handles.

  alone      every step on a handle of its own: the reference bits; the deterministic steps also against the oracle, bit for bit
             (with a low-rank update: apply to 1e-12 of the largest entry, as tests/test_lrc.py holds the update to the oracle's
             dense k x k arithmetic, and the residual = the bit-exact residual of A minus B (S o B^T y) to the same bound)
  orders     all steps on ONE handle in the listed order, its reverse and three seeded permutations: every tag equals "alone"
  twice      every step twice in a row on one handle
  intact     after every step (of every test here) every device input and every host seed array equals the copy kept before the
             first step; on the low-rank handles b_special, the right-hand side of steps of its own, carries -0.0, a denormal
             and 1e300 on support rows of the update (1e300 swamps the noise: every other step runs on an ordinary b, and its
             results are finite)
  failing    between every two steps of the listed order one call the host refuses before any launch: the documented status, and
             the results after it unchanged
  control    the comparison is shown to fail on an order-dependent step (MCSOR.set_omega(1.3), not set back)"""
import numpy as np
import pytest

import handle_steps as H
import oracle as O
import test_gpu_stream_contract as SC
from test_gpu_stream_contract import aij, ex6  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
SUBJECTS = H.subjects()
IDS = [f"{kind}-{case}" for kind, case in SUBJECTS]
ORDER_IDS = ["listed", "reversed"] + [f"perm{s}" for s in H.PERMUTATION_SEEDS]


@pytest.fixture(scope="module")
def ctx(aij, ex6):  # noqa: F811
    from parmgmc_amd import pc as P

    yield {"aij": aij, "ex6": ex6, "alone": {}, "inputs": {}}
    P.set_seed(0xCAFE)  # the library's default: the PC steps move the global seed


def same_bits(a, b):
    import torch

    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))
    if isinstance(a, np.ndarray):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, float):
        return isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b


def first_difference(got, want, order):
    """(step, tag) of the first result in call order that differs from the reference, or None"""
    for name in order:
        if name not in want:
            continue
        assert got[name].keys() == want[name].keys(), (name, sorted(got[name]), sorted(want[name]))
        for tag in got[name]:
            if not same_bits(got[name][tag], want[name][tag]):
                return name, tag
    return None


def assert_same_results(got, want, order):
    diff = first_difference(got, want, order)
    assert diff is None, f"step {diff[0]!r}, tag {diff[1]!r} differs from the step on a handle of its own; call order: {order}"


def fresh_inputs(sub, ctx):
    """clones of the subject's inputs, which are made once (the steps only read them, and run() checks that)"""
    import torch

    key = (sub.kind, sub.case)
    if key not in ctx["inputs"]:
        ctx["inputs"][key] = sub.inputs()
    return {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in ctx["inputs"][key].items()}


def run(sub, order, ctx, extra=None, between=None):
    """the results {step: {tag: value}} of the steps of `order` on one new handle; extra: further steps by name.  After every
    step, before the next one is queued: the device inputs and the host seed arrays are what they were"""
    import torch

    steps = {**{s.name: s for s in sub.steps}, **(extra or {})}
    handle, x = sub.build(), fresh_inputs(sub, ctx)
    kept = {k: v.clone() for k, v in x.items() if isinstance(v, torch.Tensor)}
    torch.cuda.synchronize()
    out = {}
    for i, name in enumerate(order):
        if between is not None and i:
            between(i, handle, x)
        assert set(steps[name].const) <= set(kept), (name, steps[name].const)
        seen = []
        with H.watch_seeds(seen):
            out[name] = steps[name].fn(handle, x)
        torch.cuda.synchronize()
        for k, v in kept.items():
            assert same_bits(x[k], v), f"step {name!r} left input {k!r} changed ({'declared const' if k in steps[name].const else 'not even an argument'}); call order: {order}"
        for arr, copy in seen:
            assert np.array_equal(arr, copy), f"step {name!r} changed its host seed array; call order: {order}"
    del handle
    return out


def alone(sub, ctx):
    """every step on a handle of its own, computed once per subject and left unchanged"""
    key = (sub.kind, sub.case)
    if key not in ctx["alone"]:
        ctx["alone"][key] = {s.name: run(sub, [s.name], ctx)[s.name] for s in sub.steps}
    return ctx["alone"][key]


# ---- alone: the reference bits, tied to the oracle where the step is deterministic ------------------------------------------------
def lowrank_apply(A, colors, lowrank, b, y):
    """MCSORApply on the MATLRC operator, forward sweep at omega 1"""
    B, S = lowrank
    Bb = O.lrc_build_correction(A, colors, B, S, 1.0, O.SOR_FORWARD)
    return O.lrc_mcsor_apply(A, colors, B, Bb, Bb, b, y, 1.0, O.SOR_FORWARD)


def lowrank_residual(plain, lowrank, y):
    B, S = lowrank
    return plain - B @ (S * (B.T @ y))


def close(got, want):
    return np.abs(SC.host(got) - want).max() <= 1e-12 * np.abs(want).max()


def mcsor_residual(A, b, y):
    """the sliced-ELL residual's order: the off-diagonal terms in storage order summed from zero, then the diagonal term, then b - sum"""
    want = np.empty(A.n)
    for i in range(A.n):
        s, d = 0.0, 0.0
        for q in range(A.rowptr[i], A.rowptr[i + 1]):
            if A.colidx[q] == i:
                d = A.vals[q] * y[i]
            else:
                s = s + A.vals[q] * y[A.colidx[q]]
        want[i] = b[i] - (s + d)
    return want


def oracle_grid(case, x, res):
    nx, ny, nz, kappa, lowrank = H.GRID_CASES[case]
    b, y = SC.host(x["b"]), SC.host(x["y"])
    assert np.array_equal(SC.host(res["to_cvec"]["from_cvec"]), b) and same_bits(res["to_cvec"]["to_cvec"], x["bc"])
    A = O.shifted_laplace(nx, ny, nz, kappa)
    if lowrank:
        want = lowrank_apply(A, O.coloring_redblack(nx, ny, nz), x["lowrank"], b, y)
        assert close(res["apply"]["apply"], want) and close(res["apply_cvec"]["apply_cvec_natural"], want)
        assert close(res["residual_cvec"]["residual"], lowrank_residual(SC.csr_residual(A, b, y), x["lowrank"], y))
        return
    want = O.mcsor_apply(A, O.coloring_redblack(nx, ny, nz), b, y, 1.0, O.SOR_FORWARD)
    assert np.array_equal(SC.host(res["apply"]["apply"]), want)
    assert np.array_equal(SC.host(res["apply_cvec"]["apply_cvec_natural"]), want)
    assert np.array_equal(SC.host(res["residual_cvec"]["residual"]), SC.csr_residual(A, b, y))


def oracle_mcsor(case, x, res):
    A, mc = H.build_mcsor(case)
    b, y, pos = SC.host(x["b"]), SC.host(x["y"]), mc.get_layout()
    assert np.array_equal(SC.host(res["to_layout"]["to_layout"])[pos], b) and np.array_equal(SC.host(res["to_layout"]["from_layout"]), y)
    Y3 = SC.host(x["Y3"])
    if x["lowrank"] is not None:
        assert close(res["apply"]["apply"], lowrank_apply(A, mc.get_coloring(), x["lowrank"], b, y))
        assert np.array_equal(SC.host(res["apply_layout"]["apply_layout"])[pos], SC.host(res["apply"]["apply"]))
        for c in range(3):
            assert close(res["apply_chains"]["apply_chains"][:, c], lowrank_apply(A, mc.get_coloring(), x["lowrank"], b, Y3[:, c])), c
        assert close(res["residual"]["residual"], lowrank_residual(mcsor_residual(A, b, y), x["lowrank"], y))
        assert np.array_equal(SC.host(res["residual_layout"]["residual_layout"])[pos], SC.host(res["residual"]["residual"]))
        return
    want = O.mcsor_apply(A, mc.get_coloring(), b, y, 1.0, O.SOR_FORWARD)
    assert np.array_equal(SC.host(res["apply"]["apply"]), want)
    assert np.array_equal(SC.host(res["apply_layout"]["apply_layout"])[pos], want)
    for c in range(3):
        assert np.array_equal(SC.host(res["apply_chains"]["apply_chains"])[:, c], O.mcsor_apply(A, mc.get_coloring(), b, Y3[:, c], 1.0, O.SOR_FORWARD)), c
    want = mcsor_residual(A, b, y)
    assert np.array_equal(SC.host(res["residual"]["residual"]), want)
    assert np.array_equal(SC.host(res["residual_layout"]["residual_layout"])[pos], want)


@pytest.mark.parametrize("kind,case", SUBJECTS, ids=IDS)
def test_alone(kind, case, ctx):
    import torch

    sub = H.subject(kind, case, ctx)
    res = alone(sub, ctx)
    assert res.keys() == {s.name for s in sub.steps}
    for name, out in res.items():
        assert out, name
        for tag, v in out.items():
            if isinstance(v, torch.Tensor) and not tag.endswith("_special"):  # (1e300 in b_special may overflow)
                assert bool(torch.isfinite(v).all()), (name, tag)
    x = fresh_inputs(sub, ctx)
    if kind == "grid":
        oracle_grid(case, x, res)
    if kind == "mcsor":
        oracle_mcsor(case, x, res)
    if kind in ("chainstats", "chaincov"):  # the read-outs, the reset and the stream setter leave the later results unchanged
        for name in res:
            for tag in res["updates"]:
                assert same_bits(res[name][tag], res["updates"][tag]), (name, tag)
    if (kind, case) in H.LOWRANK_SUBJECTS:
        assert H.has_special(SC.host(x["b_special"])) and not H.has_special(SC.host(x["b"]))
        h = sub.build()  # the form the update is kept in (the fine level's, on a hierarchy)
        k, rows, dense = h.level_lowrank_sizes(h.levels - 1) if kind.startswith("mgmc") else h.lowrank_sizes()
        assert k == 3 and rows > 0 and dense == ((kind, case) not in H.ROW_COMPACT), (k, rows, dense)
        assert dense or rows <= h.n // 4, (rows, h.n)


# ---- orders --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order_id", ORDER_IDS)
@pytest.mark.parametrize("kind,case", SUBJECTS, ids=IDS)
def test_orders(kind, case, order_id, ctx):
    sub = H.subject(kind, case, ctx)
    order = H.orders([s.name for s in sub.steps])[order_id]
    assert_same_results(run(sub, order, ctx), alone(sub, ctx), order)


# ---- twice ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,case", SUBJECTS, ids=IDS)
def test_twice(kind, case, ctx):
    sub = H.subject(kind, case, ctx)
    want = alone(sub, ctx)
    for s in sub.steps:
        again = H.Step(s.name + "_again", s.fn, s.const, s.calls)
        got = run(sub, [s.name, again.name], ctx, extra={again.name: again})
        assert_same_results({s.name: got[s.name]}, want, [s.name])
        assert_same_results({s.name: got[again.name]}, want, [s.name])


# ---- inputs intact: run() checks them after every step of every test; here the special values are shown to be in place -----------
@pytest.mark.parametrize("kind,case", H.LOWRANK_SUBJECTS, ids=[f"{k}-{c}" for k, c in H.LOWRANK_SUBJECTS])
def test_inputs_intact_with_special_values_on_support_rows(kind, case, ctx):
    sub = H.subject(kind, case, ctx)
    x = fresh_inputs(sub, ctx)
    for k in ("b_special", "bc_special", "bl_special"):  # the right-hand side in every layout the special steps hand over
        if k in x:
            assert H.has_special(SC.host(x[k])), k
    order = [s.name for s in sub.steps]
    assert_same_results(run(sub, order + order[::-1], ctx), alone(sub, ctx), order)


# ---- a failing call in between ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,case", SUBJECTS, ids=IDS)
def test_a_failing_call_in_between(kind, case, ctx):
    sub = H.subject(kind, case, ctx)
    order = [s.name for s in sub.steps]
    made = []

    def between(i, handle, x):
        f = sub.failing[(i - 1) % len(sub.failing)]
        st = f.fn(handle, x)
        made.append(f.name)
        assert st == f.status, f"{f.name}: status {st}, documented {f.status}"

    assert_same_results(run(sub, order, ctx, between=between), alone(sub, ctx), order)
    assert len(made) == len(order) - 1 and set(made) == {f.name for f in sub.failing[: len(order) - 1]}


# ---- control ---------------------------------------------------------------------------------------------------------------------
def test_control_an_order_dependent_step_fails_the_comparison(ctx):
    sub = H.subject("mcsor", "random200", ctx)
    want = alone(sub, ctx)
    leak = H.Step("set_omega_not_set_back", lambda mc, x: mc.set_omega(1.3) or {"omega": 1.3}, ["b"], [])
    order = ["residual", "to_layout", leak.name, "apply", "sample", "chains3"]  # the residual and the layout do not depend on omega
    got = run(sub, order, ctx, extra={leak.name: leak})
    assert first_difference(got, want, order) == ("apply", "apply")
    with pytest.raises(AssertionError, match="step 'apply', tag 'apply' differs"):
        assert_same_results(got, want, order)
    assert not same_bits(got["sample"]["sample"], want["sample"]["sample"]) and same_bits(got["residual"]["residual"], want["residual"]["residual"])
