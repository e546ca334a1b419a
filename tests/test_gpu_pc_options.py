"""Every option key and setter of the PC layer (parmgmc_amd/csrc/pmg_pc.c) pinned to the chain it selects: for every case of
tests/pc_option_cases.py each of three samples, read through the sample callback and finally from y, is compared with the
CPU oracle run on the configuration the REFERENCE gives those keys (tolerance of the direct-handle test of the same
operation) and, bit for bit, with the direct handle configured through its own setters -- the PC layer adds no arithmetic.
Beyond the table: the zero-guess KSP solve, prefix isolation, the stream rule, a failing sample callback, and set-up after
new operators / reset."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import pc_option_cases as T

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def rel(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


@pytest.fixture(autouse=True)
def _init():
    from parmgmc_amd import pc as P

    P.initialize()
    P.options_clear()
    P.set_seed(0xCAFE)
    yield
    P.options_clear()


def make_mat(op):
    from parmgmc_amd import pc as P

    inp = T.inputs(op)
    if inp["kind"] == "dmda":
        m = P.Mat.dmda(*inp["grid"], inp["kappa"])
    else:
        m = P.Mat.csr(inp["A"].rowptr, inp["A"].colidx, inp["A"].vals)
    return m if inp["B"] is None else m.lrc(inp["B"], inp["S"])


def apply_call(pc, name, args, inner):
    """one setter call of a case, through the Python mirror where it has the method"""
    from parmgmc_amd import pc as P

    if name == "pmg_pc_woodbury_set_sampler":
        inner["sampler"] = P.PC(args[0])
        pc.woodbury_set_sampler(inner["sampler"])
    elif name == "pmg_pc_woodbury_set_solver":
        inner["solver"] = P.PC(args[0])
        pc.woodbury_set_solver(inner["solver"])
    elif name == "pmg_pc_parsor_set_partition":
        pc.parsor_set_partition(args[0])
    else:
        getattr(pc, name[len("pmg_pc_"):])(*args)


def build_pc(c):
    """options, type, operator, "pre" setters, set_from_options, stage-0 setters, set-up: returns (pc, inner PCs handed over)"""
    from parmgmc_amd import pc as P

    for k, v in c.opts.items():
        P.options_set_value(k, v)
    pc = P.PC(c.pc or None, prefix=c.prefix)
    pc.set_operators(make_mat(c.op))
    inner = {}
    for stage, name, args in c.calls:
        if stage == "pre":
            apply_call(pc, name, args, inner)
    pc.set_from_options()
    for stage, name, args in c.calls:
        if stage == 0:
            apply_call(pc, name, args, inner)
    pc.setup()
    return pc, inner


def inner_sampler_state(pc, inner):
    """(seed, counter) of a woodbury PC's inner sampler: read from a PC that was handed over; for one made by
    -pc_woodbury_sampler the stream rule gives it -- set_from_options creates the solver, then the sampler, right after the
    outer PC (pmg_pc.c woodbury_setfromoptions), and a new PC starts at counter 0.  The C-ABI has no getter for an inner PC
    made from options, so its counter is never READ: it is held only indirectly, by the oracle chain of the samples that
    follow (a wrong seed or a counter that did not advance per draw changes sample 2 and 3, and the sample after a failing
    callback).  The direct assertion on the inner counter is made in the handed-over case."""
    if "sampler" in inner:
        return inner["sampler"].noise_state()
    return (pc.noise_state()[0] + 2 * T.STREAM_STRIDE) & M64, 0


def direct_samples(op, cfgs, seed, ctr0, y0, guesszero=False):
    """the same samples from the direct handle configured through its own setters (None where the PC has no single handle)"""
    from parmgmc_amd import MCSOR, MGMC, CholSampler, GridMCSOR, capi

    inp = T.inputs(op)
    b, out = dev(inp["b"]), []
    if isinstance(cfgs[0], T.Gibbs):
        y, ctr = dev(y0), ctr0
        for cfg in cfgs:
            if inp["kind"] == "dmda":
                h = GridMCSOR(*inp["grid"], inp["kappa"])
            else:
                rule = {"greedy": capi.COLORING_GREEDY, "lexlevels": capi.COLORING_LEXLEVELS, "iterated": capi.COLORING_ITERATED}[cfg.coloring]
                h = MCSOR(inp["A"].rowptr, inp["A"].colidx, inp["A"].vals, rule)
            h.set_omega(cfg.omega)
            h.set_sweep_type(cfg.sweep)
            if inp["kind"] != "dmda":
                h.setup()
            ctr = h.sample(b, y, 1, seed, ctr, cfg.scaled)
            out.append(host(y).copy())
            h.destroy()
        return out
    if isinstance(cfgs[0], T.MG):
        cfg = cfgs[0]
        mg = MGMC(*inp["grid"], inp["kappa"], cfg.levels)
        mg.set_smoother(cfg.scaled, cfg.omega, cfg.sweep, cfg.nu)
        mg.set_coarse("cholsampler" if cfg.coarse == "cholsampler" else "gibbs", cfg.coarse_its)
        if inp["B"] is not None:
            mg.set_lowrank(inp["B"], inp["S"])
        mg.setup()
        y = dev(y0)
        mg.sample(b, y, len(cfgs), seed, ctr0, guesszero=guesszero, callback=lambda it, yy: out.append(host(yy).copy()))
        mg.destroy()
        return out
    if isinstance(cfgs[0], T.Chol):
        ch = CholSampler(inp["A"].rowptr, inp["A"].colidx, inp["A"].vals, inp["B"], inp["S"])
        y = dev(y0)
        for it in range(len(cfgs)):
            ch.sample(b, y, seed, ctr0 + it)
            out.append(host(y).copy())
        ch.destroy()
        return out
    return None


def check_chain(c, pc, inner=None, y0=None, splits=None, direct=True):
    """run len(c.expect) samples of pc from y0 with a recording sample callback and hold every sample, the final y, the
    iteration numbers, (outits, reason) and the counter to the oracle's chain for c.expect; returns (y tensor, samples)"""
    inp = T.inputs(c.op)
    y0 = inp["y0"] if y0 is None else y0
    n = len(c.expect)
    seed, ctr0 = pc.noise_state()
    inner_state = inner_sampler_state(pc, inner or {}) if isinstance(c.expect[0], T.Woodbury) else None
    b, y = dev(inp["b"]), dev(y0)
    its_seen, seen = [], []
    pc.set_sample_callback(lambda it, yy: (its_seen.append(it), seen.append(host(yy).copy())), y)
    mid = [(name, args) for stage, name, args in c.calls if stage == 2]
    if mid:
        assert pc.apply_richardson(b, y, 2) == (2, 4)
        for name, args in mid:
            apply_call(pc, name, args, {})
        assert pc.apply_richardson(b, y, n - 2) == (n - 2, 4)  # sets itself up again; counter and callback carry on
        assert its_seen == [0, 1] + list(range(n - 2))
    else:
        assert pc.apply_richardson(b, y, n) == (n, 4)  # *outits = its; PCRICHARDSON_CONVERGED_ITS
        assert its_seen == list(range(n))
    want, ctr_end = T.expected_samples(c, seed, ctr0, y0=y0, inner=inner_state)
    tol = T.tolerance(c)
    for i, (got, w) in enumerate(zip(seen + [host(y)], want + [want[-1]])):
        err = rel(got, w)
        print(f"{c.id}: sample {min(i, n - 1)}{' (y)' if i == n else ''} vs oracle {err:.3e} (tol {tol:g})")
        assert err < tol, (c.id, i, err)
    assert pc.noise_state() == (seed, ctr_end)  # one per draw: 2 per symmetric Gibbs sample, 1 otherwise
    if inner and "sampler" in inner:
        assert inner["sampler"].noise_state() == (inner_state[0], inner_state[1] + sum(T.draws_per_sample(cfg.sampler) for cfg in c.expect))
    if direct:
        twin = direct_samples(c.op, c.expect, seed, ctr0, y0)
        if twin is not None:
            for i, (got, w) in enumerate(zip(seen + [host(y)], twin + [twin[-1]])):
                assert np.array_equal(got, w), (c.id, i, "differs from the direct handle by", np.abs(got - w).max())
    return y, seen


@pytest.mark.parametrize("c", T.CHAIN_CASES, ids=[c.id for c in T.CHAIN_CASES])
def test_case_runs_the_chain_the_reference_gives_its_keys(c):
    pc, inner = build_pc(c)
    if not c.pc:
        assert pc.get_type() == c.opts["-pc_type"]
    check_chain(c, pc, inner)


@pytest.mark.parametrize("c", T.PARSOR_CASES, ids=[c.id for c in T.PARSOR_CASES])
def test_parsor_case_applies_the_lexicographic_sweeps(c):
    """PCApply_PARSOR: cfg.its sweeps with cfg.omega from a zero guess, bit for bit the oracle's (as test_parsor_partition.py)"""
    pc, _ = build_pc(c)
    inp = T.inputs(c.op)
    y = dev(np.full(inp["A"].n, 9.0))
    pc.apply(dev(inp["b"]), y)
    want = T.expected_parsor(c.op, c.expect[0])
    assert np.array_equal(host(y), want), (c.id, np.abs(host(y) - want).max())
    assert pc.noise_state()[1] == 0  # deterministic: no draw


@pytest.mark.parametrize("cid", ["cholsampler-csr7x6", "cholsampler-lrc"])
def test_cholsampler_apply_draws_one_sample_per_call(cid):
    """PCApply_CholSampler (src/pc_chols.c:262-291): every call is one exact sample on the next counter, whatever y held"""
    c = T.BY_ID[cid]
    pc, _ = build_pc(c)
    inp = T.inputs(c.op)
    seed, ctr0 = pc.noise_state()
    want, _ = T.expected_samples(c, seed, ctr0)
    twin = direct_samples(c.op, c.expect, seed, ctr0, inp["y0"])
    y = dev(np.full(inp["A"].n, 9.0))
    for it in range(T.NSAMPLES):
        pc.apply(dev(inp["b"]), y)
        assert rel(host(y), want[it]) < T.tolerance(c) and np.array_equal(host(y), twin[it])
        assert pc.noise_state() == (seed, ctr0 + it + 1)


def test_shell_case_calls_the_apply_routine_with_its_context():
    """PCShellSetApply / SetContext / GetContext (reference examples/ex3.c:59-67,128-131) around MCSORApply"""
    from parmgmc_amd import MCSOR, capi
    from parmgmc_amd.capi import check, lib

    c = T.BY_ID["shell-set-apply-and-context"]
    cfg, inp = c.expect[0], T.inputs(c.op)
    mc = MCSOR(inp["A"].rowptr, inp["A"].colidx, inp["A"].vals).setup()
    mc.set_sweep_type(cfg.sweep)
    ctxs = []

    @capi.SHELL_APPLY
    def apply(pc_h, x_ptr, y_ptr, stream):
        got = C.c_void_p()
        st = lib.pmg_pc_shell_get_context(pc_h, C.byref(got))
        ctxs.append(got.value)
        return st or lib.pmg_mcsor_apply(mc._h, x_ptr, y_ptr, stream)

    from parmgmc_amd import pc as P

    pc = P.PC(c.pc)
    pc.set_from_options()
    (_, n1, _), (_, n2, (ctx,)) = c.calls
    assert (n1, n2) == ("pmg_pc_shell_set_apply", "pmg_pc_shell_set_context")
    check(lib.pmg_pc_shell_set_apply(pc._h, C.cast(apply, C.c_void_p)))
    check(lib.pmg_pc_shell_set_context(pc._h, C.c_void_p(ctx)))
    y = dev(inp["y0"])
    pc.apply(dev(inp["b"]), y)
    want = O.mcsor_apply(inp["A"], T.coloring(c.op, cfg.coloring), inp["b"], inp["y0"], 1.0, cfg.sweep)
    assert ctxs == [ctx] and np.array_equal(host(y), want)


ZERO_GUESS = ["mcgibbs-symmetric-omega0.7-dmda6x5x4", "sorgibbs-coloring-lexlevels-lshape", "gamgmc-default", "gamgmc-ex1-line41", "gamgmc-17x9x9-levels3", "gamgmc-lrc-mcgibbs-symmetric", "cholsampler-csr7x6", "woodbury-keys"]


@pytest.mark.parametrize("cid", ZERO_GUESS)
def test_ksp_solve_without_a_nonzero_guess_starts_from_zero(cid):
    """KSPSolve without KSPSetInitialGuessNonzero: y is zeroed whatever it held; gamgmc's first sample is then MG(b)
    (guesszero, src/pc_gamgmc.c:243-246), the others ignore the flag (src/pc_mcgibbs.c:160)"""
    c = T.BY_ID[cid]
    pc, inner = build_pc(c)
    inp = T.inputs(c.op)
    n = inp["A"].n
    seed, ctr0 = pc.noise_state()
    inner_state = inner_sampler_state(pc, inner) if isinstance(c.expect[0], T.Woodbury) else None
    y = dev(np.full(n, 9.0))
    pc.ksp_solve(dev(inp["b"]), y, T.NSAMPLES, guess_nonzero=False)
    want, ctr_end = T.expected_samples(c, seed, ctr0, y0=np.zeros(n), guesszero=True, inner=inner_state)
    err = rel(host(y), want[-1])
    print(f"{cid}: zero-guess solve vs oracle {err:.3e}")
    assert err < T.tolerance(c) and pc.noise_state() == (seed, ctr_end)
    twin = direct_samples(c.op, c.expect, seed, ctr0, np.zeros(n), guesszero=True)
    if twin is not None:
        assert np.array_equal(host(y), twin[-1])


def gibbs_case(op, cfg, pc="mcgibbs"):
    return T.case(f"{pc}-{op}", pc, op, expect=cfg)


def test_prefixed_keys_reach_only_their_own_pc():
    from parmgmc_amd import pc as P

    P.options_set_value("-a_pc_mcgibbs_omega", "1.3")
    P.options_set_value("-b_pc_mcgibbs_symmetric", "")
    P.options_set_value("-pc_mcgibbs_omega", "0.7")  # unprefixed: reaches neither
    P.options_set_value("-pc_mcgibbs_backward", "")
    op = "dmda6x5x4"
    pcs = {}
    for pre in ("a_", "b_"):
        pcs[pre] = P.PC("mcgibbs", prefix=pre)
        pcs[pre].set_operators(make_mat(op))
        pcs[pre].set_from_options()
    check_chain(gibbs_case(op, T.Gibbs(True, 1.3, T.FWD, "redblack")), pcs["a_"])
    check_chain(gibbs_case(op, T.Gibbs(True, 1.0, T.SYM, "redblack")), pcs["b_"])
    late = P.PC("mcgibbs")  # the prefix given after creation counts too
    late.set_options_prefix("a_")
    late.set_operators(make_mat(op))
    late.set_from_options()
    check_chain(gibbs_case(op, T.Gibbs(True, 1.3, T.FWD, "redblack")), late)


def test_every_pc_has_its_own_noise_stream_by_creation_order():
    """seed of a PC = pmg_seed + 0xD1B54A32D192ED03 * (id + 1) mod 2^64 with ids handed out in creation order; pmg_set_seed
    moves every PC; each PC's chain is the oracle's with its own seed"""
    from parmgmc_amd import pc as P

    inv = pow(T.STREAM_STRIDE, -1, 1 << 64)
    P.set_seed(1234)
    a, b = P.PC("mcgibbs"), P.PC("mcgibbs")
    ids = [(((pc.noise_state()[0] - 1234) * inv) & M64) - 1 for pc in (a, b)]
    assert ids[1] == ids[0] + 1 and 0 <= ids[0] < 1 << 32
    P.set_seed(0xFFFFFFFFFFFFFFF0)  # wraps modulo 2^64
    seeds = [pc.noise_state()[0] for pc in (a, b)]
    assert seeds == [(0xFFFFFFFFFFFFFFF0 + T.STREAM_STRIDE * (i + 1)) & M64 for i in ids] and seeds[0] != seeds[1]
    op = "dmda9x9"
    ys = []
    for pc in (a, b):
        pc.set_operators(make_mat(op))
        ys.append(check_chain(gibbs_case(op, T.Gibbs(True, 1.0, T.FWD, "redblack")), pc)[1][-1])
    assert rel(ys[0], ys[1]) > 1e-6  # two streams, two chains


FAILING = ["mcgibbs-default-dmda9x9", "mcgibbs-symmetric-dmda9x9", "sorgibbs-default-csr7x6", "gamgmc-nu2", "gamgmc-default", "cholsampler-csr7x6", "woodbury-keys"]


@pytest.mark.parametrize("cid", FAILING)
def test_chain_resumes_after_a_failing_sample_callback(cid):
    """a sample callback returning 77 at it == 1: the call returns 77, y is sample 1, the counter stands behind sample 1, and
    the next call draws sample 2 -- not sample 0's or 1's noise again"""
    from parmgmc_amd import capi
    from parmgmc_amd.capi import lib
    from parmgmc_amd.wrappers import _ptr, _stream

    c = T.BY_ID[cid]
    pc, inner = build_pc(c)
    inp = T.inputs(c.op)
    seed, ctr0 = pc.noise_state()
    inner_state = inner_sampler_state(pc, inner) if isinstance(c.expect[0], T.Woodbury) else None
    want, _ = T.expected_samples(c, seed, ctr0, inner=inner_state)
    _, ctr2 = T.expected_samples(c._replace(expect=c.expect[:2]), seed, ctr0, inner=inner_state)
    its_seen = []

    @capi.SAMPLE_CALLBACK
    def cb(it, _y, _n, _ctx):
        its_seen.append(it)
        return 77 if it == 1 else 0

    capi.check(lib.pmg_pc_set_sample_callback(pc._h, cb, None, None))
    b, y = dev(inp["b"]), dev(inp["y0"])
    outits, reason = C.c_int32(-1), C.c_int32(-1)
    st = lib.pmg_pc_apply_richardson(pc._h, _ptr(b), _ptr(y), T.NSAMPLES, 0, C.byref(outits), C.byref(reason), _stream())
    assert st == 77 and its_seen == [0, 1]
    tol = T.tolerance(c)
    assert rel(host(y), want[1]) < tol
    assert pc.noise_state() == (seed, ctr2)
    its_seen.clear()
    assert pc.apply_richardson(b, y, 1) == (1, 4) and its_seen == [0]
    err = rel(host(y), want[2])
    print(f"{cid}: resumed sample 2 vs oracle {err:.3e}")
    assert err < tol
    assert pc.noise_state() == (seed, T.expected_samples(c, seed, ctr0, inner=inner_state)[1])


RESETUP = {"mcgibbs-omega1.3-dmda9x9": "dmda9x9b", "sorgibbs-coloring-lexlevels-csr7x6": "csr7x6b", "gamgmc-ex1-line41": "mg9x9b", "cholsampler-csr7x6": "csr7x6b"}


@pytest.mark.parametrize("cid", sorted(RESETUP))
def test_new_operators_and_reset_set_the_pc_up_again(cid):
    """after three samples: pmg_pc_reset alone, then one sample -- the PC keeps its operator and options, sets itself up again
    and draws the oracle's next sample from the old y at the counter the chain had reached; pmg_pc_set_operators with another
    operator of the same size, one sample -- the oracle's for the new operator; and reset once more on that operator"""
    c = T.BY_ID[cid]
    pc, _ = build_pc(c)
    y, seen = check_chain(c, pc)
    for step, op in (("reset", c.op), ("set_operators", RESETUP[cid]), ("reset", RESETUP[cid])):
        if step == "reset":
            pc.reset()  # nothing else: no set_operators, no set_from_options
        else:
            pc.set_operators(make_mat(op))
        one = c._replace(id=f"{cid}-after-{step}-on-{op}", op=op, expect=c.expect[:1])
        y, seen = check_chain(one, pc, y0=seen[-1])
