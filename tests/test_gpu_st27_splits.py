"""The class-stencil level kernels (st27_pair_phase_kernel, st27_pair_residual_kernel and the per-colour kernels they replace)
at every way split_pairs cuts a line and at every position of a plane's last line tile: the shapes of st27_splits.py, which
test_st27_splits.py pins to their branches without a GPU.

st27_split_workloads.py runs in a fresh child per switch setting (the PMG_* switches are read once per process): default,
PMG_ST27_PACK_REMAINDER=0, PMG_ST27_PAIR=0, and PMG_ST27_PAIR=0 with the plane kernel on every level.  INSIDE the child every
row is compared with the oracle -- deterministic forward and backward sweeps, the residual and the Q1 transfers bit for bit,
noisy sweeps (seed above 2^32, non-zero counter) within 1e-13 of the largest entry, the stencil table within 1e-13 of the
oracle's Galerkin product -- for (scaled = False, omega = 1) and (scaled = True, omega = 1.3), plus a three-level, a
semicoarsened and a flat hierarchy for the transfers between class-stencil levels, the generic transfers and the XCD-run form
of the quad prolongation.  Here: every vector of the other settings equals the default's bit for bit; whole V-cycle chains
on four hierarchies whose class-stencil level has a tabled line length against oracle_chain at 1e-11 (the tolerance of
test_gpu_mgmc.py: Galerkin entries and residual sums are taken in another order); negative controls; and, with rocprofv3 on
PATH, which kernels ran with which grid sizes, from the restated rule."""
import csv
import functools
import os
import re
import shutil
import subprocess
import sys
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import oracle as O
import st27_split_workloads as W
import st27_splits as M
from mgmc_oracle import oracle_chain, oracle_hierarchy
from test_gpu_vcycle_shapes_oracle import SETTINGS

HERE = Path(__file__).resolve().parent
CHILD = HERE / "st27_split_workloads.py"
CHILD_TIMEOUT = 300  # s; a child takes seconds beyond the start of torch
VCYCLE_TOL = 1e-11

CONFIGS = {
    "default": {},
    "pack_remainder_0": {"PMG_ST27_PACK_REMAINDER": "0"},
    "pair_0": {"PMG_ST27_PAIR": "0"},
    "pair_0_plane_all": {"PMG_ST27_PAIR": "0", "PMG_ST27_PHASE_MAX_PLANE": "1000000000"},
}
PACKED_SHAPE, UNPACKED_SHAPE = (121, 17, 3), (199, 15, 4)  # negative controls: sweep remainder 1 packed 12 to a wavefront; 60 + 40 pairs


def _trace(d):
    """kernel name -> Counter of grid sizes in work-items, over every dispatch in a rocprofv3 --kernel-trace csv under d"""
    files = sorted(Path(d).rglob("*kernel_trace.csv"))
    assert files, f"rocprofv3 wrote no kernel_trace.csv under {d}"
    out = {}
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                out.setdefault(row["Kernel_Name"], Counter())[(int(row["Grid_Size_X"]), int(row["Grid_Size_Y"]), int(row["Grid_Size_Z"]))] += 1
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """config -> (results, kernel launches or None); the children run one after the other, the first that fails stops the fixture"""
    tmp = tmp_path_factory.mktemp("st27_splits")
    prof = shutil.which("rocprofv3")
    base = {k: v for k, v in os.environ.items() if not k.startswith("PMG_") or k == "PMG_LIBRARY"}
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    done = {}
    for name, cenv in CONFIGS.items():
        out, tdir = tmp / f"{name}.npz", tmp / f"trace_{name}"
        cmd = py + [str(CHILD), str(out)]
        if prof:
            cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", str(tdir), "--"] + cmd
        p = subprocess.run(cmd, env=dict(base, **cenv), cwd=str(HERE.parent), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        if p.returncode != 0 or not out.exists():
            pytest.fail(f"child {name} exited with {p.returncode}; stderr:\n{p.stderr[-4000:]}")
        print(f"--- child {name} ---\n{p.stdout}")
        with np.load(out) as z:
            res = {k: z[k] for k in z.files}
        done[name] = (res, _trace(tdir) if prof else None)
        if prof:
            shutil.rmtree(tdir)
    return done


# ---- values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_default_child_ran_every_comparison(runs):
    res, _ = runs["default"]
    per_level = {"in/coef", "in/sqrtd", "in/b", "in/y0", "det_fwd", "det_bwd", "noisy_fwd", "noisy_bwd", "resid"}
    for dims in M.SHAPES:
        for si in range(len(W.SMOOTHERS)):
            assert {f"{W.key(dims)}/s{si}/{k}" for k in per_level} <= set(res)
        want = {"restrict", "prolong"} | ({"fused_rr"} if dims[2] > 1 else set())
        assert {k.split("/")[1] for k in res if k.startswith(W.key(dims) + "/") and k.count("/") == 1} == want
    assert {"three/st27/restrict", "three/st27/prolong", "three/grid/fused_rr", "semi/grid/restrict", "semi/grid/prolong", "quad/grid/prolong"} <= set(res)
    assert "semi/grid/fused_rr" not in res
    assert sum(k.startswith("vcycle/") for k in res) == len(M.VCYCLE_SHAPES) * (len(SETTINGS) + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("config", [c for c in CONFIGS if c != "default"])
def test_switch_settings_give_the_default_bits(runs, config):
    import torch

    (ref, _), (res, _) = runs["default"], runs[config]
    assert sorted(res) == sorted(ref)
    differ = [k for k in sorted(ref) if not torch.equal(torch.from_numpy(res[k]), torch.from_numpy(ref[k]))]
    assert not differ, f"{len(differ)} of {len(ref)} vectors differ from the default's, first {differ[:5]}"
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in res.values())
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in ref.values())


@functools.lru_cache(maxsize=None)
def _hierarchy(grid, levels):
    return oracle_hierarchy(*grid, W.KAPPA, levels)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS) + ["guesszero"])
@pytest.mark.parametrize("grid", list(M.VCYCLE_SHAPES), ids=[W.key(g) for g in M.VCYCLE_SHAPES])
def test_vcycle_chain_matches_oracle(runs, grid, setting):
    """three samples from a non-zero start under the four settings of test_gpu_vcycle_shapes_oracle.py, and from the zero
    guess: the only way into the zero-guess instantiations of the paired sweep and the one-colour prolongation"""
    levels, gz = M.VCYCLE_SHAPES[grid], setting == "guesszero"
    scaled, omega, sweep, nu, coarse, cits, _ = SETTINGS["default" if gz else setting]
    b, y0 = W.vcycle_inputs(grid)
    n = len(b)
    got = runs["default"][0][f"vcycle/{W.key(grid)}/{setting}"].reshape(W.VCYCLE_ITS, n)
    want = oracle_chain(grid, W.KAPPA, levels, b, np.zeros(n) if gz else y0, W.VCYCLE_ITS, W.VCYCLE_SEED, W.VCYCLE_COUNTER0, gz, nu=nu, scaled=scaled,
                        omega=omega, sweep=sweep, coarse=coarse, coarse_its=cits, lv=_hierarchy(grid, levels))
    for it, (g, w) in enumerate(zip(got, want)):
        err = np.abs(g - w).max() / np.abs(w).max()
        print(f"{grid} {setting} sample {it}: {err:.3e}")
        assert err < VCYCLE_TOL, f"sample {it}: {err:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [PACKED_SHAPE, UNPACKED_SHAPE], ids=["packed", "unpacked"])
def test_the_comparison_notices_a_wrong_direction_and_a_wrong_draw(runs, dims):
    """negative controls: the oracle with the sweep direction flipped is not the deterministic sweep, and with the counter moved
    by one it is more than 100 tolerances from the noisy sweep"""
    assert M.sweep_split(PACKED_SHAPE[0]).packed and not M.sweep_split(UNPACKED_SHAPE[0]).packed
    res, _ = runs["default"]
    cx, cy, cz = dims
    N, off = cx * cy * cz, cx * cy
    rows = np.arange(N, dtype=np.int64)
    for si, (scaled, omega) in enumerate(W.SMOOTHERS):
        v = lambda k: res[f"{W.key(dims)}/s{si}/{k}"]  # noqa: E731
        coef, sqrtd, b, y0 = v("in/coef"), v("in/sqrtd"), v("in/b"), v("in/y0")
        for backward, d in ((False, "fwd"), (True, "bwd")):
            y1 = v(f"det_{d}")[off:off + N]
            assert np.array_equal(y1, O.st27_rows_sweep(cx, cy, cz, coef, sqrtd, rows, b, y0, y1, omega=omega, backward=backward))
            assert not np.array_equal(y1, O.st27_rows_sweep(cx, cy, cz, coef, sqrtd, rows, b, y0, y1, omega=omega, backward=not backward))
            y1 = v(f"noisy_{d}")[off:off + N]
            far = O.st27_rows_sweep(cx, cy, cz, coef, sqrtd, rows, b, y0, y1, omega=omega, backward=backward, noisy=True, seed=W.SEED_BIG, sweep=W.COUNTER + 1)
            assert np.abs(y1 - far).max() > 100 * W.NOISE_TOL * np.abs(far).max()


# ---- kernels -----------------------------------------------------------------------------------------------------------------
def _level_runs():
    """the class-stencil levels whose kernels the child runs one by one: each once forward and once backward without noise"""
    out = [dims for dims in M.SHAPES for _ in W.SMOOTHERS]
    return out + M.st27_levels(*M.THREE_LEVEL, True) + M.st27_levels(*M.SEMICOARSENED, True)


def _vcycle_levels():
    """(first coarse levels, coarsest levels under coarse = gibbs) of the V-cycle hierarchies"""
    return list(M.VCYCLE_LEVELS), [M.st27_levels(g, l, True)[-1] for g, l in M.VCYCLE_SHAPES.items()]


PAIR_SWEEP = re.compile(r"st27_pair_phase_kernel<(\w+), (\w+), (\w+), (\w+), (\w+)>")


def _pair_sweeps(launches):
    """(noisy, backward, zero-guess, packed) -> Counter of workgroups of the paired sweep's launches"""
    out = {}
    for name, grids in launches.items():
        m = PAIR_SWEEP.search(name)
        if not m:
            continue
        noisy, backward, zin, _, pack = (g == "true" for g in m.groups())
        for (gx, gy, gz), cnt in grids.items():
            assert gx % 64 == 0 and (gy, gz) == (M.PT + 1, 1), (name, gx, gy, gz)
            out.setdefault((noisy, backward, zin, pack), Counter())[gx // 64] += cnt
    return out


def _named(launches, pattern):
    """Counter of grid sizes over the kernels whose name matches"""
    out = Counter()
    for name, grids in launches.items():
        if re.search(pattern, name):
            out.update(grids)
    return out


def _expected_pair(pack):
    """deterministic launches as a multiset per (backward, packed); the workgroup counts of the noisy ones as a set per packed"""
    det = {(bw, pk): Counter() for bw in (False, True) for pk in (False, True)}
    for dims in _level_runs():
        for packed, wg in M.sweep_launches(*dims, pack=pack):
            for bw in (False, True):
                det[(bw, packed)][wg] += 1
    first, coarsest = _vcycle_levels()
    noisy = {pk: {wg for dims in _level_runs() + first + coarsest for packed, wg in M.sweep_launches(*dims, pack=pack) if packed == pk} for pk in (False, True)}
    return det, noisy


def _check_pair_sweeps(launches, pack):
    got, (det, noisy) = _pair_sweeps(launches), _expected_pair(pack)
    for bw in (False, True):
        for pk in (False, True):
            assert got.get((False, bw, False, pk), Counter()) == det[(bw, pk)], f"deterministic sweeps, backward {bw}, packed {pk}"
            assert not got.get((False, bw, True, pk)), "a deterministic sweep from a zero guess"
    for pk in (False, True):
        seen = set()
        for (nz, bw, zin, p), c in got.items():
            if nz and p == pk:
                seen |= set(c)
        assert seen == noisy[pk], f"noisy sweeps, packed {pk}: workgroups {sorted(seen)} for {sorted(noisy[pk])}"
    assert any(nz and zin for nz, _, zin, _ in got), "no V-cycle sweep started from a zero guess"


def _check_pair_residuals(launches, pack):
    first, coarsest = _vcycle_levels()
    for pk in (False, True):
        got = _named(launches, r"st27_pair_residual_kernel<%s>" % ("true" if pk else "false"))
        sure = {(64 * wg, M.RESID_TILE, 1) for dims in _level_runs() + first for packed, wg in M.residual_launches(*dims, pack=pack) if packed == pk}
        maybe = {(64 * wg, M.RESID_TILE, 1) for dims in coarsest for packed, wg in M.residual_launches(*dims, pack=pack) if packed == pk}
        assert sure <= set(got) <= sure | maybe, f"residual, packed {pk}: {sorted(got)} for {sorted(sure)}"
    # the level residuals alone as a multiset would need the V-cycles' count; their packed share is what the switch removes
    assert bool(_named(launches, r"st27_pair_residual_kernel<true>")) == pack


def _check_per_colour(launches, limit):
    """PMG_ST27_PAIR=0: the plane kernel for planes of at most `limit` points, one launch per colour above"""
    assert not _named(launches, r"st27_pair_phase_kernel") and not _named(launches, r"st27_pair_residual_kernel")
    plane, colour = Counter(), Counter()
    for dims in _level_runs():
        if M.plane_kernel(*dims[:2], limit=limit):
            for wg in M.plane_launches(*dims):
                plane[(1024 * wg, 1, 1)] += 2  # forward and backward
        else:
            for wg, planes in M.color_launches(*dims):
                colour[(256 * wg, 1, planes)] += 2
    assert _named(launches, r"st27_phase_kernel<false>") == plane
    assert _named(launches, r"st27_color_sweep_kernel<false>") == colour
    first, coarsest = _vcycle_levels()
    every = _level_runs() + first + coarsest
    assert set(_named(launches, r"st27_phase_kernel<true>")) == {(1024 * wg, 1, 1) for d in every if M.plane_kernel(*d[:2], limit=limit) for wg in M.plane_launches(*d)}
    assert set(_named(launches, r"st27_color_sweep_kernel<true>")) == {(256 * wg, 1, p) for d in every if not M.plane_kernel(*d[:2], limit=limit) for wg, p in M.color_launches(*d)}
    return plane, colour


@pytest.mark.gpu
def test_kernels_and_grid_sizes_are_the_restated_rule(runs):
    traces = {name: t for name, (_, t) in runs.items()}
    if traces["default"] is None:
        pytest.skip("rocprofv3 not on PATH: the values were compared, the kernel names and grid sizes were not")
    # default: the packed instantiations exactly where the rule packs, with its workgroup counts
    _check_pair_sweeps(traces["default"], True)
    _check_pair_residuals(traces["default"], True)
    assert not _named(traces["default"], r"st27_phase_kernel") and not _named(traces["default"], r"st27_color_sweep_kernel")
    # PMG_ST27_PACK_REMAINDER=0: none of them, every remainder a segment of the one-line-per-wavefront launch
    assert not _named(traces["pack_remainder_0"], r"st27_pair_phase_kernel<\w+, \w+, \w+, \w+, true>")
    _check_pair_sweeps(traces["pack_remainder_0"], False)
    _check_pair_residuals(traces["pack_remainder_0"], False)
    # PMG_ST27_PAIR=0: the plane kernel up to 1100 points per plane, the per-colour kernel above; both occur
    plane, colour = _check_per_colour(traces["pair_0"], M.PLANE_LIMIT)
    assert plane and colour
    # ... with the plane kernel on every level: no per-colour launch, planes of more than 1024 points among them
    plane, colour = _check_per_colour(traces["pair_0_plane_all"], 10 ** 9)
    assert plane and not colour and not _named(traces["pair_0_plane_all"], r"st27_color_sweep_kernel")
    # the quad prolongation of the flat hierarchy in its XCD-run form: 66 blocks padded to 72, two plane pairs and two colours
    fine = M.FLAT_QUAD[0]
    nb, padded = M.quad_prolong_blocks(*fine[:2])
    assert padded > nb >= 64
    for t in traces.values():
        assert (256 * padded, 1, 2 * ((fine[2] + 1) // 2)) in _named(t, r"q1_prolong_add_quad_kernel")
        assert _named(t, r"st27_restrict_full_kernel") and _named(t, r"st27_prolong_add_cell_kernel")  # between class-stencil levels
