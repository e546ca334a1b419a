"""Every PMG_* environment switch the native library reads is documented in INTEGRATION.md section 5, and every switch
there that claims to leave results alone is held to that by a test: a configuration of test_gpu_switches.py, or the
existing test named in PINNED_ELSEWHERE (which must mention the switch)."""
import re
from pathlib import Path

from test_gpu_switches import CONFIGS

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "parmgmc_amd" / "csrc"

# diagnostics: read by the library, change no arithmetic
DIAGNOSTIC = {
    "PMG_TRACE": "ROCTx ranges around sweeps and noise fills",
    "PMG_IPC_DEBUG": "prints flag words to stderr after a failed wait",
}
# timing probes that need not be documented in section 5 (none at present)
PROBES = {}
# result-path switches pinned by tests outside test_gpu_switches.py
PINNED_ELSEWHERE = {
    "PMG_LRC_DENSE": "tests/test_lrc.py",
    "PMG_LRC_FUSED": "tests/test_gpu_lrc_fused.py",
    "PMG_LRC_RESTORE": "tests/test_gpu_lrc_fused.py",
    "PMG_LRC_REDUCE": "tests/test_gpu_lrc_fused.py",
    "PMG_LRC_BATCH": "tests/test_gpu_lrc_fused.py",
    "PMG_LRC_BTY": "tests/test_gpu_lrc_fused.py",
    "PMG_MG_FULL_GALERKIN": "tests/test_gpu_mgmc.py",
    "PMG_MG_REPLICATE_BELOW": "tests/test_gpu_dist_two_ranks.py",
    "PMG_ST27_PAIR_SLAB": "tests/test_gpu_dist_two_ranks.py",
    "PMG_GRID_FUSED_RR_SLAB": "tests/test_gpu_dist_two_ranks.py",
    "PMG_DISTMCSOR_REFRESH_BY_COLOUR": "tests/test_gpu_rowblock_c.py",
}


def native_switches():
    names = set()
    for f in sorted(CSRC.glob("*.c")) + sorted(CSRC.glob("*.hip")):
        names |= set(re.findall(r'getenv\(\s*"(PMG_[A-Z0-9_]+)"', f.read_text()))
    return names


def section5():
    text = (ROOT / "INTEGRATION.md").read_text()
    m = re.search(r"^## 5\..*?(?=^## 6\.)", text, re.S | re.M)
    assert m, "INTEGRATION.md has no section 5"
    return m.group(0)


def switches_under_test():
    return {k for env, _ in CONFIGS.values() for k in env}


def test_the_scan_finds_the_switches():
    found = native_switches()
    assert {"PMG_GRID_TAIL", "PMG_ST27_PAIR", "PMG_SELL_LOCALITY", "PMG_GRID_SX_ALIGN"} <= found
    assert all(n in found for n in DIAGNOSTIC) and all(n in found for n in PINNED_ELSEWHERE)


def test_every_native_switch_is_documented():
    documented = set(re.findall(r"`(PMG_[A-Z0-9_]+)", section5()))
    missing = sorted(native_switches() - documented - set(PROBES))
    assert not missing, f"read by the library, not in INTEGRATION.md section 5: {missing}"


def test_every_result_path_switch_is_pinned():
    under_test = switches_under_test()
    loose = sorted(n for n in native_switches() - set(DIAGNOSTIC) - set(PROBES) if n not in under_test and n not in PINNED_ELSEWHERE)
    assert not loose, f"no A/B test holds these switches to the default results: {loose}"
    for name, test in PINNED_ELSEWHERE.items():
        assert name in (ROOT / test).read_text(), f"{test} does not exercise {name}"


def test_switch_table_names_only_real_switches():
    assert not sorted(switches_under_test() - native_switches())
