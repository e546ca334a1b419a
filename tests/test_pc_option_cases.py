"""The table of tests/pc_option_cases.py checked without a device: its cases separate in the oracle (so the tolerance of
tests/test_gpu_pc_options.py cannot hide an ignored option), it covers every option key pmg_pc.c reads and every PC setter
the header declares, and the option / setter failures that need no device return the reference's statuses."""
import ctypes as C
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

import pc_option_cases as T

ROOT = Path(__file__).resolve().parent.parent
SEED, CTR0, INNER = 0xCAFE, 5, (0xBEEF, 0)
SEPARATION = 1e-6  # relative; five orders above the loosest oracle tolerance the GPU module uses (1e-11; 1e-10 on MATLRC)


@pytest.fixture(scope="module")
def third_samples():
    """third sample of every chain case in the oracle alone, computed once per distinct (operator, configuration)"""
    memo, out = {}, {}
    for c in T.CHAIN_CASES:
        key = (c.op, c.expect)
        if key not in memo:
            memo[key] = T.expected_samples(c, SEED, CTR0, inner=INNER)[0][-1]
        out[c.id] = memo[key]
    return out


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_cases_with_different_reference_semantics_separate_in_the_oracle(third_samples):
    equal = {frozenset(p) for p in T.EQUAL_PAIRS}
    groups = {}
    for c in T.CHAIN_CASES:
        groups.setdefault((c.op, c.pc or c.opts["-pc_type"]), []).append(c)
    npairs, close = 0, []
    for cases in groups.values():
        for a, b in itertools.combinations(cases, 2):
            if a.expect == b.expect or frozenset((a.id, b.id)) in equal:
                continue
            npairs += 1
            d = rel(third_samples[a.id], third_samples[b.id])
            if not d >= SEPARATION:
                close.append((a.id, b.id, d))
    assert not close, "\n".join(map(str, close))
    assert npairs > 100, npairs  # (the comparison is not vacuous)


def test_pairs_listed_as_equal_are_equal_in_the_oracle(third_samples):
    for a, b in T.EQUAL_PAIRS:
        ca, cb = T.BY_ID[a], T.BY_ID[b]
        assert ca.op == cb.op and ca.expect != cb.expect, (a, b)  # a listed pair reads differently ...
        assert np.array_equal(third_samples[a], third_samples[b]), (a, b)  # ... and is one chain
    # cases with the same configuration are the same chain by construction of the builders (one computation per configuration)
    # the identity behind the pairs, on the oracle's own sweep: scaled noise at omega 1 is the unscaled noise, bit for bit
    import oracle as O

    inp = T.inputs("lshape")
    noise = lambda d: O.noise_rows(inp["A"].n, SEED, d)  # noqa: E731
    s = [O.gibbs_samples(inp["A"], T.coloring("lshape", "greedy"), inp["b"], inp["y0"], 2, noise, 1.0, O.SOR_SYMMETRIC, scaled) for scaled in (True, False)]
    assert np.array_equal(s[0], s[1])


def test_mid_chain_setter_cases_continue_from_the_old_sample(third_samples):
    """sample 3 of a set-between-samples case is neither the chain with the old parameter nor the one with the new from the start"""
    for op in ("dmda9x9", "lshape"):
        mid = third_samples[f"mcgibbs-set-omega-mid-{op}"]
        assert rel(mid, third_samples[f"mcgibbs-default-{op}"]) > SEPARATION and rel(mid, third_samples[f"mcgibbs-omega0.7-{op}"]) > SEPARATION


# ----------------------------------------------------------------------------------------------------------------
# coverage of the table against the source
# ----------------------------------------------------------------------------------------------------------------
def option_lookups():
    """the argument text of every opt_find / opt_bool / opt_real / opt_int call in pmg_pc.c (not their four definitions)"""
    text = (ROOT / "parmgmc_amd" / "csrc" / "pmg_pc.c").read_text()
    out = []
    for m in re.finditer(r"(?<!static const char \*)(?<!static int )\bopt_(?:find|bool|real|int)\(", text):
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        out.append(text[m.end():i - 1])
    return out


def option_keys_read_by_the_pc_layer():
    return {k for args in option_lookups() for k in re.findall(r'"(-[a-z_]+)"', args)}


def test_the_scan_finds_the_keys():
    keys = option_keys_read_by_the_pc_layer()
    assert {"-pc_type", "-pc_mcgibbs_omega", "-pc_sorgibbs_coloring", "-pc_mcgibbs_coloring", "-mg_coarse_ksp_max_it", "-pc_woodbury_sampler", "-pc_parsor_its", "-mg_coarse_pc_mcgibbs_symmetric", "-mg_levels_pc_mcgibbs_forward"} <= keys
    calls = option_lookups()
    assert len(calls) >= 25 and all(re.search(r'"-[a-z_]+"', a) or a.startswith("prefix, name") for a in calls), [a for a in calls if '"-' not in a]  # every lookup names its key in place


# the prefixes a key of pmg_pc.c is looked up under: the PC's own (a case's `prefix`), then "gamgmc_" for the keys of the
# inner multigrid (src/pc_gamgmc.c:285-287) or the inner Woodbury prefixes (src/woodbury.c:195,209)
INNER_PREFIXES = ("", "pc_woodbury_solver_", "pc_woodbury_sampler")


def case_reads(c, key):
    """does case c set exactly `key` (a key of pmg_pc.c, e.g. "-pc_mcgibbs_omega" or "-mg_levels_ksp_max_it") on a PC of the
    type that reads it?"""
    if key.startswith("-mg_") or key == "-pc_mg_levels":
        return c.pc == "gamgmc" and f"-{c.prefix}gamgmc_{key[1:]}" in c.opts
    owner = re.match(r"-pc_(mcgibbs|sorgibbs|parsor|gamgmc|woodbury)_", key)
    for inner in INNER_PREFIXES:
        if f"-{c.prefix}{inner}{key[1:]}" in c.opts:
            if inner:
                return c.pc == "woodbury" and c.expect is not None
            return owner is None or c.pc == owner.group(1)
    return False


def test_every_option_key_of_the_pc_layer_is_in_the_table():
    keys = option_keys_read_by_the_pc_layer()
    missing = sorted(k for k in keys if not any(case_reads(c, k) for c in T.CASES))
    assert not missing, f"read by pmg_pc.c, set by no case of tests/pc_option_cases.py on the PC that reads it: {missing}"
    # the stand-alone keys are covered by stand-alone cases, not only through a woodbury PC's inner sampler
    for k in ("-pc_mcgibbs_omega", "-pc_mcgibbs_forward", "-pc_mcgibbs_backward", "-pc_mcgibbs_symmetric", "-pc_parsor_omega"):
        assert any(k in c.opts and c.pc == k.split("_")[1] for c in T.CASES), k
    assert not case_reads(T.BY_ID["gamgmc-levels-omega1.2"], "-pc_mcgibbs_omega") and not case_reads(T.BY_ID["woodbury-keys"], "-pc_type")


def test_every_pc_setter_of_the_header_is_in_the_table():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "parmgmc_hip.h").read_text(), flags=re.S)
    setters = set(re.findall(r"\b(pmg_pc_[a-z]+_set_[a-z_]+)\s*\(", header))
    assert {"pmg_pc_mcgibbs_set_omega", "pmg_pc_gamgmc_set_levels", "pmg_pc_woodbury_set_sampler"} <= setters
    called = {name for c in T.CASES for _, name, _ in c.calls}
    assert not sorted(setters - called), f"declared, in no case: {sorted(setters - called)}"
    assert not sorted(called - setters), f"called by a case, not declared: {sorted(called - setters)}"


# ----------------------------------------------------------------------------------------------------------------
# error paths that need no device
# ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def P():
    from parmgmc_amd import pc as P

    P.initialize()
    P.options_clear()
    yield P
    P.options_clear()


def make_mat(P, op):
    inp = T.inputs(op)
    if inp["kind"] == "dmda":
        m = P.Mat.dmda(*inp["grid"], inp["kappa"])
    else:
        m = P.Mat.csr(inp["A"].rowptr, inp["A"].colidx, inp["A"].vals)
    return m if inp["B"] is None else m.lrc(inp["B"], inp["S"])


def call_setter(P, pc, name, args, keep):
    """the status of one setter call of a case (no exception: the table names the status)"""
    from parmgmc_amd.capi import lib

    if name in ("pmg_pc_woodbury_set_sampler", "pmg_pc_woodbury_set_solver"):
        inner = P.PC(args[0])
        st = getattr(lib, name)(pc._h, inner._h)
        if st == 0:
            inner._borrowed = True  # the woodbury PC owns it now
        keep.append(inner)
        return st
    if name == "pmg_pc_parsor_set_partition":
        rs = np.ascontiguousarray(args[0], np.int32)
        return lib.pmg_pc_parsor_set_partition(pc._h, len(rs) - 1, rs.ctypes.data, None)
    if name == "pmg_pc_shell_set_apply":
        return lib.pmg_pc_shell_set_apply(pc._h, None)
    if name == "pmg_pc_shell_set_context":
        return lib.pmg_pc_shell_set_context(pc._h, C.c_void_p(args[0]))
    return getattr(lib, name)(pc._h, *args)


@pytest.mark.parametrize("c", T.ERROR_CASES, ids=[c.id for c in T.ERROR_CASES])
def test_option_and_setter_failures_return_the_reference_status(c, P):
    from parmgmc_amd.capi import lib

    for k, v in c.opts.items():
        P.options_set_value(k, v)
    pc = P.PC(c.pc or None, prefix=c.prefix)
    pc.set_operators(make_mat(P, c.op))
    status, where = c.error
    keep = []
    st = lib.pmg_pc_set_from_options(pc._h)
    if where == "set_from_options":
        assert st == status, (st, lib.pmg_last_error_string())
        for key in (k for k in c.opts if "mg_coarse_pc_mcgibbs" in k):
            assert key.encode() in lib.pmg_last_error_string()  # the message names the key that cannot be honoured
        return
    assert st == 0
    got = [call_setter(P, pc, name, args, keep) for _, name, args in c.calls if name == where]
    assert got == [status], (got, lib.pmg_last_error_string())


def test_failed_set_type_leaves_an_untyped_pc(P):
    """pmg_pc_set_type destroys the old implementation before it looks the new type up: after a failed lookup the PC has
    no type, and nothing may reach through the old one"""
    from parmgmc_amd.capi import lib

    pc = P.PC("mcgibbs")
    pc.set_operators(make_mat(P, "dmda9x9"))
    assert lib.pmg_pc_set_type(pc._h, b"no_such_pc") == T.UNKNOWN_TYPE
    assert pc.get_type() == ""
    assert lib.pmg_pc_mcgibbs_set_omega(pc._h, 1.3) == T.ARG_WRONG
    assert lib.pmg_pc_mcgibbs_set_sweep_type(pc._h, 2) == T.ARG_WRONG
    assert lib.pmg_pc_setup(pc._h) == T.WRONGSTATE
    assert lib.pmg_pc_set_from_options(pc._h) == 0  # nothing to configure
    pc.set_type("sorgibbs")
    assert pc.get_type() == "sorgibbs"
    assert lib.pmg_pc_set_from_options(pc._h) == 0


def test_options_of_a_valid_case_are_accepted_without_a_device(P):
    """set_from_options of every non-error case succeeds (set-up, which needs the device, is not called)"""
    from parmgmc_amd.capi import lib

    for c in T.CASES:
        if c.error is not None:
            continue
        P.options_clear()
        for k, v in c.opts.items():
            P.options_set_value(k, v)
        pc = P.PC(c.pc or None, prefix=c.prefix)
        pc.set_operators(make_mat(P, c.op))
        keep = []
        for stage, name, args in c.calls:
            if stage == "pre":
                assert call_setter(P, pc, name, args, keep) == 0
        assert lib.pmg_pc_set_from_options(pc._h) == 0, (c.id, lib.pmg_last_error_string())
        if not c.pc:
            assert pc.get_type() == c.opts["-pc_type"]
