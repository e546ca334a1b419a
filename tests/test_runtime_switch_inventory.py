"""Every PMG_* environment switch the native library reads is a row of the table in csrc/pmg_switch.c, which alone reads the
environment, and is documented in INTEGRATION.md section 5, and every switch there that claims to leave results alone is
held to that by a test: a configuration of test_gpu_switches.py, or the existing test named in PINNED_ELSEWHERE (which
must mention the switch)."""
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
    "PMG_GRID_PLANE_PAIR": "tests/test_gpu_grid_plane_pair.py",
}


def table_rows():
    """(id, name) of every row of the switch table: `[PMG_SW_X] = {"PMG_X", kind, default, read time}`"""
    return re.findall(r'^\s*\[(PMG_SW_[A-Z0-9_]+)\]\s*=\s*\{"(PMG_[A-Z0-9_]+)",', (CSRC / "pmg_switch.c").read_text(), re.M)


def native_switches():
    return {name for _, name in table_rows()}


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


def test_only_the_table_reads_the_environment():
    for d in (CSRC, ROOT / "include", ROOT / "examples"):
        for f in sorted(p for p in d.rglob("*") if p.is_file() and p.suffix in (".c", ".h", ".hip", ".hpp", ".inc", ".cpp")):
            if f == CSRC / "pmg_switch.c":
                continue
            text = f.read_text()
            assert not re.search(r"getenv\s*\([^)]*PMG_", text), f"{f.name} reads a PMG_ variable by itself"
            if d == CSRC:  # nor through a name held elsewhere: a switch of the library is a row of the table
                assert not re.search(r"getenv\s*\(", text), f"{f.name} calls getenv"
    # the table passes its names to getenv and holds no name outside its rows
    text = (CSRC / "pmg_switch.c").read_text()
    assert text.count("getenv(") == 1 and "getenv(pmg_switch_row[id].name)" in text
    assert len(re.findall(r'"PMG_[A-Z0-9_]+"', text)) == len(table_rows())


def test_ids_and_rows_correspond_one_to_one():
    header = (CSRC / "pmg_switch.h").read_text()
    ids = re.findall(r"PMG_SW_[A-Z0-9_]+", re.search(r"typedef enum \{(.*?)\} pmg_switch_id;", header, re.S).group(1))
    assert ids[-1] == "PMG_SW_COUNT" and len(set(ids)) == len(ids)
    rows = table_rows()
    assert [i for i, _ in rows] == ids[:-1], "one row per id, in the order of the enum"
    assert all(name == "PMG_" + i[len("PMG_SW_"):] for i, name in rows) and len({n for _, n in rows}) == len(rows)
