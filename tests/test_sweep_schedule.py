"""The sweep schedule of the host layer (pmg_sweep_iter, pmg_sweep_color, pmg_sweep_ndir in csrc/pmg_internal.h and the
per-level sweep counts in csrc/pmg_mgmc_internal.h) against the Python statement of the same contract
(capi.directions, dist.color_schedule).  tests/sanitize/sweep_schedule.c is compiled with gcc
-fsanitize=address,undefined and prints what the helpers give; no device, nothing preloaded."""
import shutil
import subprocess
from pathlib import Path

import pytest

from parmgmc_amd.capi import SOR_BACKWARD_SWEEP, SOR_FORWARD_SWEEP, SOR_SYMMETRIC_SWEEP, directions
from parmgmc_amd.dist import color_schedule

ROOT = Path(__file__).resolve().parent.parent
TYPES = (SOR_FORWARD_SWEEP, SOR_BACKWARD_SWEEP, SOR_SYMMETRIC_SWEEP)
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    exe = tmp_path_factory.mktemp("sweep_schedule") / "sweep_schedule"
    cmd = [gcc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", str(ROOT / "tests" / "sanitize" / "sweep_schedule.c"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}, timeout=60)
    assert run.returncode == 0 and run.stdout.endswith("sweep_schedule ok\n"), (run.stdout[-2000:], run.stderr[-4000:])
    out = {}
    for line in run.stdout.splitlines()[:-1]:
        key, _, val = line.partition(" :")
        assert key not in out, key
        out[key] = val.strip()
    return out


def test_iterator_follows_directions(printed):
    n = 0
    for t in TYPES:
        for its in (0, 1, 3):
            for noisy in (0, 1):
                for c0 in (0, 5, 2**32 - 1, 2**64 - 2):
                    dirs = [d for _ in range(its) for d in directions(t)]
                    steps = " ".join(f"{d}:{(c0 + i) & M64}" for i, d in enumerate(dirs))
                    ctr = (c0 + len(dirs)) & M64 if noisy else c0
                    assert printed[f"S {t} {its} {noisy} {c0}"] == f"{steps} ; {ctr}".strip(), (t, its, noisy, c0)
                    n += 1
    assert n == 72 and sum(k.startswith("S ") for k in printed) == n


def test_ndir_and_colour_order(printed):
    for t in TYPES:
        assert printed[f"N {t}"] == str(len(directions(t)))
    for d in (SOR_FORWARD_SWEEP, SOR_BACKWARD_SWEEP):
        for nc in (1, 2, 5):
            order = list(range(nc)) if d == SOR_FORWARD_SWEEP else list(range(nc - 1, -1, -1))
            assert printed[f"C {d} {nc}"] == " ".join(map(str, order))
        # the two-colour grids: what the slab drivers take from dist.color_schedule
        assert tuple(map(int, printed[f"C {d} 2"].split())) == color_schedule(d)[0]
    assert [tuple(map(int, printed[f"C {d} 2"].split())) for d in directions(SOR_SYMMETRIC_SWEEP)] == color_schedule(SOR_SYMMETRIC_SWEEP)


def test_directional_sweeps_of_a_level_per_cycle(printed):
    n = 0
    for t in TYPES:
        ndir = len(directions(t))
        for nu in (1, 2):
            for coarse_type in (0, 1):
                for coarse_its in (1, 3):
                    for l in (0, 1, 2):
                        leg = nu * ndir if l >= 1 else (coarse_its * ndir if coarse_type else 0)
                        cycle = 2 * leg if l >= 1 else leg  # pre- and post-smoothing above the coarsest level
                        assert printed[f"L {t} {nu} {coarse_type} {coarse_its} {l}"] == f"{leg} {cycle}"
                        n += 1
    assert n == 72
