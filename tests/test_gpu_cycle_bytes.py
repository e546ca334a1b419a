"""pmg_mgmc_get_algorithmic_bytes -- the byte model bench.py divides by the measured time for every V-cycle roofline
line -- pinned to tests/golden/cycle_bytes.json (tools/record_cycle_bytes.py, whose list of configurations this module
imports) with EXACT equality: every term is a product of integers held in doubles far below 2^53.  And the model
follows the kernel path the cycle takes where a process-wide switch decides it."""
import json
import os
import subprocess
import sys

import pytest

from tools import record_cycle_bytes as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("group", R.GROUPS, ids=R.group_name)
def test_bytes_equal_the_recorded_ones(group):
    with open(R.FIXTURE) as f:
        want = json.load(f)
    got = R.group_bytes(group)
    assert len(got) == len(R.TOGGLES) and set(got) <= set(want)
    for name, (total, per) in got.items():
        print(name, total, per)
        assert [total, per] == want[name], name


def test_fixture_holds_exactly_the_listed_configurations():
    with open(R.FIXTURE) as f:
        want = json.load(f)
    assert sorted(want) == sorted("%s_%s_%s" % (R.group_name(g), form, tr) for g in R.GROUPS for form, tr in R.TOGGLES)


def _child_bytes(body, **env):
    """algorithmic_bytes() lines printed by a 33^3 / 3-level hierarchy in a child process (the switches are per process)"""
    code = (
        "import json, os, sys, torch; sys.path.insert(0, %r); from parmgmc_amd import MGMC;"
        "mg = MGMC(33, 33, 33, 5.0, 3).setup();"
        "show = lambda: print(json.dumps([mg.algorithmic_bytes()[0], mg.algorithmic_bytes()[1].tolist()]));"
    ) % ROOT + body
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, check=True).stdout
    return [json.loads(line) for line in out.splitlines() if line.startswith("[")]


def test_bytes_follow_a_refused_fused_kernel():
    """PMG_GRID_FUSED_RR=0: the fused residual + restriction refuses every level, the cycle launches residual, then
    restriction -- the same two kernels as under set_fused_transfers(False), so the same bytes"""
    (refused,) = _child_bytes("show()", PMG_GRID_FUSED_RR="0")
    (unfused, fused) = _child_bytes("mg.set_fused_transfers(False); show(); mg.set_fused_transfers(True); show()")
    print(refused, unfused, fused)
    assert unfused != fused
    assert refused == unfused


def test_bytes_keep_the_prolongation_the_cycle_latched():
    """PMG_MG_PROLONG_BOTH is read once per process: set after the first sample it changes neither the cycle nor the
    bytes reported for it"""
    before, after = _child_bytes(
        "b = torch.ones(33**3, dtype=torch.float64, device='cuda'); y = torch.zeros_like(b);"
        "show(); mg.sample(b, y, 1, seed=3); os.environ['PMG_MG_PROLONG_BOTH'] = '1'; show()"
    )
    print(before, after)
    assert before == after
