"""The switch table of the native library (csrc/pmg_switch.c, csrc/pmg_switch.h) against the expressions its call sites
used before there was a table: for every switch CASES holds that expression over the string getenv returned (None:
unset) and what the call site now makes of the accessor's value; the two agree on every string of VALUES.
tests/sanitize/switch_table.c is compiled together with pmg_switch.c with gcc -fsanitize=address,undefined (and once more
with -fsanitize=thread for eight racing first reads) and prints what the accessors return; no device, nothing preloaded."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
VALUES = (None, "", "0", "1", "2", "3", "4", "16", "400", "1000000000", "x")


def atoll(s, bits=64):
    """C's atoll (strtoll, base 10) on a string; atoi is the same cut to 32 bits, as glibc does it"""
    m = re.match(r"[ \t\n\v\f\r]*([+-]?)(\d*)", s)
    v = int(m.group(2) or "0") * (-1 if m.group(1) == "-" else 1)
    v = max(-(2**63), min(2**63 - 1, v))  # strtoll saturates
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def atoi(s):
    return atoll(s, 32)


def int_or(dflt):  # e ? atoi(e) : dflt
    return lambda e: atoi(e) if e is not None else dflt


def present(e):  # getenv(..) != NULL
    return int(e is not None)


def c0(e):  # e[0] of a C string, 0 for the terminator
    return ord(e[0]) if e else 0


def same(v, _set):
    return v


# name -> (the parent commit's expression over the string, what the call site makes of (accessor value, is-set flag))
CASES = {
    "PMG_GRID_PACKED": (int_or(2), same),
    "PMG_GRID_BANDED": (int_or(1), same),
    "PMG_GRID_TAIL": (int_or(1), same),
    "PMG_GRID_FLAT": (int_or(1), same),
    "PMG_GRID_PLANE_PAIR": (int_or(1), same),
    # static const int off = getenv(..) ? !atoi(getenv(..)) : 0
    "PMG_GRID_FUSED_RR": (lambda e: int(not atoi(e)) if e is not None else 0, lambda v, s: int(not v)),
    "PMG_GRID_RR_CHUNK": (int_or(0), same),
    "PMG_GRID_RR_SYNC": (int_or(-1), same),
    "PMG_TRANSFER_GENERIC": (present, same),
    "PMG_ST27_PHASE_MAX_PLANE": (int_or(1100), same),
    "PMG_ST27_PACK_REMAINDER": (int_or(1), same),
    "PMG_ST27_PAIR": (int_or(1), same),
    "PMG_ST27_PAIR_SLAB": (int_or(1), same),
    "PMG_MG_FUSED_ZERO": (int_or(1), same),
    "PMG_MG_PROLONG_BOTH": (present, same),
    "PMG_SELL_LOCALITY": (int_or(1), same),
    "PMG_DISTMCSOR_REFRESH_BY_COLOUR": (present, same),
    # force = env && env[0] == '1'; off = env && env[0] == '0'
    "PMG_TRACE": (lambda e: (e is not None and c0(e) == ord("1"), e is not None and c0(e) == ord("0")), lambda v, s: (v == ord("1"), v == ord("0"))),
    # al = e ? atoi(e) : <the size rule>
    "PMG_GRID_SX_ALIGN": (lambda e: atoi(e) if e is not None else "size rule", lambda v, s: v if s else "size rule"),
    # the fused form applies unless getenv(..) && !atoi(getenv(..))
    "PMG_GRID_FUSED_RR_SLAB": (lambda e: not (e is not None and not atoi(e)), lambda v, s: bool(v)),
    # rep = 2^19; if (getenv(..)) rep = atoll(getenv(..))
    "PMG_MG_REPLICATE_BELOW": (lambda e: atoll(e) if e is not None else 1 << 19, same),
    "PMG_MG_FULL_GALERKIN": (present, same),
    "PMG_MG_NO_STENCIL": (present, same),
    "PMG_MG_CSR_TRANSFERS": (present, same),
    # unfused = !(e && e[0] == '1'); unfused_rhs = !(e && (e[0] == '1' || e[0] == '2')); unfused_restore = !(e && (e[0] == '1' || e[0] == '3'))
    "PMG_LRC_FUSED": (
        lambda e: (not (e is not None and c0(e) == ord("1")), not (e is not None and c0(e) in (ord("1"), ord("2"))), not (e is not None and c0(e) in (ord("1"), ord("3")))),
        lambda v, s: (v != ord("1"), v != ord("1") and v != ord("2"), v != ord("1") and v != ord("3")),
    ),
    "PMG_LRC_RESTORE": (lambda e: not (e is not None and c0(e) == ord("0")), lambda v, s: v != ord("0")),
    "PMG_LRC_REDUCE": (lambda e: not (e is not None and c0(e) == ord("0")), lambda v, s: v != ord("0")),
    "PMG_LRC_BTY": (lambda e: e is not None and c0(e) == ord("1"), lambda v, s: v == ord("1")),
    "PMG_LRC_DENSE": (present, same),
    # eta_batch_mode = (e && !atoi(e)) ? -1 : 1
    "PMG_LRC_BATCH": (lambda e: -1 if e is not None and not atoi(e) else 1, lambda v, s: 1 if v else -1),
    "PMG_IPC_DEBUG": (present, same),
}
WIDE = {"PMG_MG_REPLICATE_BELOW"}  # read with pmg_switch_wide; every other site takes the int


def _build(tmp_path_factory, sanitizer, *more):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    exe = tmp_path_factory.mktemp("switch_table") / "switch_table"
    cmd = [gcc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-fno-omit-frame-pointer", f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all", "-pthread", *more, str(ROOT / "tests" / "sanitize" / "switch_table.c"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, *args):
    env = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "TSAN_OPTIONS": "halt_on_error=1", "PATH": "/usr/bin:/bin"}
    run = subprocess.run([str(exe), *args], capture_output=True, text=True, env=env, timeout=60)
    assert run.returncode == 0 and run.stdout.endswith("switch_table ok\n") and not run.stderr, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    out = {}
    for line in run.stdout.splitlines()[:-1]:
        key, _, val = line.partition(" :")
        assert key not in out, key
        out[key] = val.split()
    return out


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    return _run(_build(tmp_path_factory, "address,undefined"))


@pytest.fixture(scope="module")
def raced(tmp_path_factory):
    return _run(_build(tmp_path_factory, "thread"), "threads")


def _rows(printed):
    return {key.split()[2]: key.split()[3] for key in printed if key.startswith("V 0 ")}


def test_the_atoi_emulation():
    assert [atoi(s) for s in VALUES[1:]] == [0, 0, 1, 2, 3, 4, 16, 400, 1000000000, 0]
    assert atoi(" -12x") == -12 and atoi("+7") == 7 and atoi("4294967296") == 0 and atoll("4294967296") == 2**32 and atoll("9" * 30) == 2**63 - 1


def test_every_row_is_a_case(printed):
    assert set(_rows(printed)) == set(CASES) and len(CASES) == 31
    assert sum(k.startswith("V ") for k in printed) == len(VALUES) * len(CASES)


def test_every_switch_on_every_string_as_the_parent_read_it(printed):
    for name, (parent, site) in CASES.items():
        for i, e in enumerate(VALUES):
            wide, narrow, is_set = map(int, printed[f"V {i} {name} {_rows(printed)[name]}"])
            assert is_set == (e is not None), (name, e)
            assert site(wide if name in WIDE else narrow, is_set) == parent(e), (name, e, wide, narrow)


def test_process_rows_latch_one_by_one(printed):
    got = {k[2:]: int(v[0]) for k, v in printed.items() if k.startswith("P ")}
    # all variables "0", PACKED read; all "1", PACKED and (for the first time) BANDED read; all unset, both and (first) TAIL read
    assert got == {"PMG_GRID_PACKED first": 0, "PMG_GRID_PACKED after_setenv": 0, "PMG_GRID_BANDED first": 1, "PMG_GRID_PACKED after_unsetenv": 0, "PMG_GRID_BANDED after_unsetenv": 1, "PMG_GRID_TAIL first": 1}
    assert _rows(printed)["PMG_GRID_PACKED"] == _rows(printed)["PMG_GRID_BANDED"] == _rows(printed)["PMG_GRID_TAIL"] == "PROCESS"


def test_live_rows_follow_every_change(printed):
    live = {n for n, when in _rows(printed).items() if when == "LIVE"}
    assert {k[2:] for k in printed if k.startswith("L ")} == live
    for name in live:
        parent, site = CASES[name]
        got = list(map(int, printed[f"L {name}"]))
        for v, e in zip(got, ("1", "0", None, "2", ""), strict=True):  # the sequence switch_table.c sets, one read after each
            assert site(v, e is not None) == parent(e), (name, e, got)
        assert len(set(got)) > 1, (name, got)  # it moved
        assert got[2] == int(printed[f"V 0 {name} LIVE"][0])  # unset again: the default


def test_the_live_switches_are_the_ones_the_integration_guide_names(printed):
    text = (ROOT / "INTEGRATION.md").read_text()
    sec5 = re.search(r"^## 5\..*?(?=^## 6\.)", text, re.S | re.M).group(0)
    m = re.search(r"read\s+at\s+every\s+use:(.*?)\.\s", sec5, re.S)
    assert m, "section 5 has no list of the switches read at every use"
    assert set(re.findall(r"`(PMG_[A-Z0-9_]+)`", m.group(1))) == {n for n, when in _rows(printed).items() if when == "LIVE"}


def test_eight_threads_first_read_every_process_row_at_once(raced, printed):
    process = {n for n, when in _rows(printed).items() if when == "PROCESS"}
    assert {k[2:] for k in raced} == process and len(process) == 18
    for name in process:  # every variable is "3"; the program has checked that the eight threads agree
        parent, site = CASES[name]
        v = int(raced[f"T {name}"][0])
        assert site(v, 1) == parent("3"), (name, v)
