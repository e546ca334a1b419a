"""The host part of the coloured block Gibbs sampler (csrc/pmg_blockgibbs_host.c) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/sanitize/blockgibbs_host.c, a stand-alone program with its own main, is compiled together
with that one file (gcc -fsanitize=address,undefined, -ffp-contract=off as the library's Makefile) and run as an executable.
It checks colour validity and the first-fit rule, that interior and exterior entries partition every block row, the packing,
||A_PP - L L^T|| and ||W L - I|| against classical bounds, and every error path.  No device, nothing preloaded.

The handle's own state errors need no device either and are checked here through the C-ABI."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_host_part_under_sanitizers(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    exe = tmp_path / "blockgibbs_host"
    srcs = [ROOT / "tests" / "sanitize" / "blockgibbs_host.c", ROOT / "parmgmc_amd" / "csrc" / "pmg_blockgibbs_host.c"]
    cmd = [gcc, "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", *map(str, srcs), "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}, timeout=120)
    assert run.returncode == 0 and run.stdout.endswith("blockgibbs_host ok\n"), (run.stdout[-2000:], run.stderr[-4000:])


def test_handle_state_errors_without_a_device():
    from parmgmc_amd.capi import lib

    rp, ci = np.array([0, 2, 4], np.int32), np.array([0, 1, 0, 1], np.int32)
    v = np.array([2.0, -1.0, -1.0, 2.0])
    bp, br = np.array([0, 2], np.int32), np.array([0, 1], np.int32)
    h = C.c_void_p()
    assert lib.pmg_blockgibbs_create_csr(2, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 1, bp.ctypes.data, br.ctypes.data, None) == 85
    assert lib.pmg_blockgibbs_create_csr(2, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 1, bp.ctypes.data, br.ctypes.data, C.byref(h)) == 0
    n, d, t = C.c_int32(), C.c_double(), C.c_int()
    # before set-up: getters and sweeps are in the wrong state (as pmg_mcsor's), checked before any device work
    assert lib.pmg_blockgibbs_get_num_colors(h, C.byref(n)) == 73
    assert lib.pmg_blockgibbs_get_coloring(h, br.ctypes.data) == 73
    assert lib.pmg_blockgibbs_get_num_slots(h, C.byref(n)) == 73
    assert lib.pmg_blockgibbs_get_block_factor(h, 0, C.byref(n), None) == 73
    assert lib.pmg_blockgibbs_get_algorithmic_bytes(h, C.byref(d)) == 73
    assert lib.pmg_blockgibbs_apply(h, 8, 8, None) == 73
    assert lib.pmg_blockgibbs_sample(h, 8, 8, 1, 0, 0, None, None) == 73
    assert lib.pmg_blockgibbs_sweep_xi(h, 0, 8, 8, 8, None) == 73
    assert b"pmg_blockgibbs_setup" in lib.pmg_last_error_string()
    assert lib.pmg_blockgibbs_apply(h, None, 8, None) == 85
    assert lib.pmg_blockgibbs_sample(h, 8, 8, -1, 0, 0, None, None) == 63
    # sweep types as pmg_mcsor (reference src/mc_sor.c:427)
    assert lib.pmg_blockgibbs_set_sweep_type(h, 4) == 56
    for typ in (1, 2, 3):
        assert lib.pmg_blockgibbs_set_sweep_type(h, typ) == 0
        assert lib.pmg_blockgibbs_get_sweep_type(h, C.byref(t)) == 0 and t.value == typ
    assert lib.pmg_blockgibbs_set_layout(h, 1, br.ctypes.data) == 63  # ld < n
    assert lib.pmg_blockgibbs_set_coloring(h, -1, br.ctypes.data) == 63
    assert lib.pmg_blockgibbs_destroy(C.byref(h)) == 0 and not h.value
    assert lib.pmg_blockgibbs_destroy(C.byref(h)) == 0  # destroying NULL is a no-op
    # create-time block errors
    big = np.arange(65, dtype=np.int32)
    assert lib.pmg_blockgibbs_create_csr(2, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 1, np.array([0, 65], np.int32).ctypes.data, big.ctypes.data, C.byref(h)) == 56
    assert not h.value
    assert lib.pmg_blockgibbs_create_csr(2, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 1, np.array([0, 0], np.int32).ctypes.data, br.ctypes.data, C.byref(h)) == 63
    assert lib.pmg_blockgibbs_create_csr(2, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 1, bp.ctypes.data, np.array([0, 2], np.int32).ctypes.data, C.byref(h)) == 63
    assert lib.pmg_blockgibbs_create_csr(2, rp.ctypes.data, ci.ctypes.data, v.ctypes.data, 1, bp.ctypes.data, np.array([1, 1], np.int32).ctypes.data, C.byref(h)) == 63
