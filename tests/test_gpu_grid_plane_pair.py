"""The plane-pair form of the noisy red-black grid sweep (grid_color_pair_sweep_kernel: one wavefront sweeps a line of two
consecutive planes and shares the same-line rows between them) against the one-plane kernel, which PMG_GRID_PLANE_PAIR=0
restores (the noise-free sweep keeps the one-plane kernel either way and is compared all the same): the same chains in a fresh child process per setting (plane_pair_workloads.py), every colour vector equal bit
for bit -- noisy and deterministic, omega = 1 and 1.3, forward, backward and symmetric sweeps, three sweeps from a
non-zero start, a seed above 2^32.

The shapes of the "plain" group are small (a lone plane, one pair, odd plane and line counts, line ends inside and just
behind a wavefront); by default their lines would be packed into wavefronts or have their tails collected, which keeps the
one-plane kernel, so both children of that group run with PMG_GRID_PACKED=0 and PMG_GRID_TAIL=0.  The "default" group runs
under the default switches: XCD bands and the flat walk with plane pairs, a slab with plane ranges, and a tail-mapped
shape.  With rocprofv3 on PATH the children run under its kernel trace, and which kernel ran is asserted as well."""
import csv
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
CHILD = HERE / "plane_pair_workloads.py"
CHILD_TIMEOUT = 180  # s; a child takes seconds beyond the start of torch

PAIR = r"grid_color_pair_sweep_kernel<\w+>"
ONE_PLAIN = r"grid_color_sweep_kernel<\w+, \w+, false, false, false>"
ONE_TAIL = r"grid_color_sweep_kernel<\w+, \w+, false, false, true>"
ONE_NOISY = r"grid_color_sweep_kernel<true, "
PLAIN_ENV = {"PMG_GRID_PACKED": "0", "PMG_GRID_TAIL": "0"}


def _trace(d):
    """(kernel name, grid size in work-items) of every dispatch in a rocprofv3 --kernel-trace csv under d"""
    files = sorted(Path(d).rglob("*kernel_trace.csv"))
    assert files, f"rocprofv3 wrote no kernel_trace.csv under {d}"
    out = set()
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                out.add((row["Kernel_Name"], (int(row["Grid_Size_X"]), int(row["Grid_Size_Y"]), int(row["Grid_Size_Z"]))))
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(group, pair on) -> (results, kernel launches or None); the first child that fails stops the fixture"""
    tmp = tmp_path_factory.mktemp("plane_pair")
    prof = shutil.which("rocprofv3")
    base = {k: v for k, v in os.environ.items() if not k.startswith("PMG_") or k == "PMG_LIBRARY"}
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    done = {}
    for group, genv in (("plain", PLAIN_ENV), ("default", {})):
        for on in (False, True):
            out, tdir = tmp / f"{group}_{int(on)}.npz", tmp / f"trace_{group}_{int(on)}"
            cmd = py + [str(CHILD), group, str(out)]
            if prof:
                cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", str(tdir), "--"] + cmd
            env = dict(base, **genv, **({} if on else {"PMG_GRID_PLANE_PAIR": "0"}))
            p = subprocess.run(cmd, env=env, cwd=str(HERE.parent), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
            if p.returncode != 0 or not out.exists():
                pytest.fail(f"child {group} (pair {'on' if on else 'off'}) exited with {p.returncode}; stderr:\n{p.stderr[-4000:]}")
            with np.load(out) as z:
                res = {k: z[k] for k in z.files}
            done[(group, on)] = (res, _trace(tdir) if prof else None)
            if prof:
                shutil.rmtree(tdir)
    return done


def _matching(launches, pattern):
    rx = re.compile(pattern)
    return {(k, g) for k, g in launches if rx.search(k)}


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["plain", "default"])
def test_plane_pairs_give_the_one_plane_bits(runs, group):
    import torch

    (ref, _), (res, _) = runs[(group, False)], runs[(group, True)]
    assert sorted(res) == sorted(ref) and len(ref) >= 12 * 5
    differ = [k for k in sorted(ref) if not torch.equal(torch.from_numpy(res[k]), torch.from_numpy(ref[k]))]
    assert not differ, f"{len(differ)} of {len(ref)} colour vectors differ from the one-plane kernel's, first {differ[:5]}"
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in ref.values())


@pytest.mark.gpu
def test_plane_pair_kernel_is_selected_where_stated(runs):
    (_, off_plain), (_, on_plain) = runs[("plain", False)], runs[("plain", True)]
    (_, off_dflt), (_, on_dflt) = runs[("default", False)], runs[("default", True)]
    if on_plain is None:
        pytest.skip("rocprofv3 not on PATH: the bits were compared, the kernel names were not")
    # switch off: the one-plane kernel alone
    assert not _matching(off_plain, PAIR) and not _matching(off_dflt, PAIR)
    assert _matching(off_plain, ONE_PLAIN) and _matching(off_dflt, ONE_PLAIN) and _matching(off_dflt, ONE_TAIL)
    # default, plain group: every noisy sweep is a plane-pair launch, omega = 1 and omega != 1
    assert not _matching(on_plain, ONE_NOISY), sorted(_matching(on_plain, ONE_NOISY))[:3]
    assert len({k for k, _ in _matching(on_plain, PAIR)}) == 2
    # default switches: the tail-mapped 257 x 257 x 4 keeps the one-plane kernel (its noisy sweeps are the only ones left on
    # it), the others pair their planes -- the z extent of a launch counts pairs: 170 x 64 x 4 in XCD bands of 8 lines is (8 x 64, 2 x 4, 2)
    assert _matching(on_dflt, ONE_TAIL) and _matching(on_dflt, ONE_NOISY) <= _matching(on_dflt, ONE_TAIL)
    assert any(g == (512, 8, 2) for _, g in _matching(on_dflt, PAIR)), sorted(g for _, g in _matching(on_dflt, PAIR))


def test_the_switch_is_read_and_documented():
    """PMG_GRID_PLANE_PAIR is a row of the library's switch table, the grid launcher reads that row, and INTEGRATION.md
    section 5 lists it (what test_runtime_switch_inventory.py asks of every row; the A/B above is what holds this one to the
    default's bits)"""
    csrc = HERE.parent / "parmgmc_amd" / "csrc"
    assert re.search(r'^\s*\[PMG_SW_GRID_PLANE_PAIR\]\s*=\s*\{"PMG_GRID_PLANE_PAIR",', (csrc / "pmg_switch.c").read_text(), re.M)
    assert "pmg_switch(PMG_SW_GRID_PLANE_PAIR)" in (csrc / "kernels_grid.hip").read_text()
    sec5 = re.search(r"^## 5\..*?(?=^## 6\.)", (HERE.parent / "INTEGRATION.md").read_text(), re.S | re.M).group(0)
    assert "`PMG_GRID_PLANE_PAIR=0`" in sec5
