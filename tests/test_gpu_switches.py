"""Every result-path runtime switch of INTEGRATION.md section 5, A/B against the defaults: the same workloads
(switch_workloads.py) run in a fresh child process per configuration -- the switches are read once per process -- and
every result must be the default child's, byte for byte.

A byte-equal A/B test also passes when a switch does nothing (a renamed variable, a shape that never reaches the
branch).  So each configuration names the difference it must make: with rocprofv3 on PATH the children run under its
kernel trace and the launches must differ from the default child's as stated in CONFIGS; layout switches show
themselves in the child's own "meta/" facts.  SHAPE_BRANCHES (grid_mappings.py) records which thread mapping each part-A
shape (test_gpu_vcycle_shapes_oracle.py) and each GridMCSOR-only shape of the child reaches on its grid level, checked
against the default child's trace, as is the launch of the in-kernel halo kernel on the plain unpacked mapping.

The children run one after another, each with a time limit; the first one that fails stops the fixture."""
import csv
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from grid_mappings import HALO_TRACE_GSIZE, HALO_TRACE_SHAPE, SHAPE_BRANCHES, sweep_mapping

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
CHILD = HERE / "switch_workloads.py"
CHILD_TIMEOUT = 420  # s; a child takes well under a minute (torch start-up, set-up of the config-4 hierarchy)

SWEEP_TAIL = r"grid_color_sweep_kernel<\w+, \w+, false, false, true>"
SWEEP_PACKED = r"grid_color_sweep_kernel<\w+, \w+, false, true, false>"
SWEEP_PLAIN = r"grid_color_sweep_kernel<\w+, \w+, false, false, false>"
SWEEP_HALO_PLAIN = r"grid_color_sweep_kernel<\w+, \w+, true, false, false>"

# configuration -> (environment, [(kind, pattern)]).  Kinds, each against the default child:
#   gone: a kernel matching the pattern ran in the default child and not here;  new: the reverse;
#   absent: none ran here;  launches: the set of (kernel, grid size) of the matching kernels differs;
#   meta: the child's "meta/" facts under this prefix differ (checked with or without rocprofv3).
CONFIGS = {
    "default": ({}, []),
    "grid_tail_0": ({"PMG_GRID_TAIL": "0"}, [("gone", SWEEP_TAIL), ("gone", r"grid_residual_kernel<false, true>")]),
    "grid_packed_0": ({"PMG_GRID_PACKED": "0"}, [("gone", SWEEP_PACKED), ("gone", r"grid_residual_kernel<true, false>")]),
    "grid_packed_1": ({"PMG_GRID_PACKED": "1"}, [("gone", SWEEP_PLAIN), ("launches", SWEEP_PACKED)]),
    "grid_banded_0": ({"PMG_GRID_BANDED": "0"}, [("launches", r"grid_color_sweep_kernel"), ("launches", r"grid_residual_kernel")]),
    "grid_flat_0": ({"PMG_GRID_FLAT": "0"}, [("launches", r"grid_color_sweep_kernel")]),
    "grid_sx_align_16": ({"PMG_GRID_SX_ALIGN": "16"}, [("meta", "meta/cvec/")]),
    "grid_sx_align_4": ({"PMG_GRID_SX_ALIGN": "4"}, [("meta", "meta/cvec/")]),
    "grid_fused_rr_0": ({"PMG_GRID_FUSED_RR": "0"}, [("gone", r"grid_residual_restrict_kernel")]),
    "grid_rr_chunk_1": ({"PMG_GRID_RR_CHUNK": "1"}, [("launches", r"grid_residual_restrict_kernel")]),
    "grid_rr_chunk_3": ({"PMG_GRID_RR_CHUNK": "3"}, [("launches", r"grid_residual_restrict_kernel")]),
    "grid_rr_sync_0": ({"PMG_GRID_RR_SYNC": "0"}, [("gone", r"grid_residual_restrict_kernel<true>")]),
    "grid_rr_sync_1": ({"PMG_GRID_RR_SYNC": "1"}, [("gone", r"grid_residual_restrict_kernel<false>")]),
    "st27_pair_0": ({"PMG_ST27_PAIR": "0"}, [("gone", r"st27_pair_phase_kernel"), ("new", r"st27_phase_kernel"), ("new", r"st27_color_sweep_kernel")]),
    "st27_pair_0_plane_0": ({"PMG_ST27_PAIR": "0", "PMG_ST27_PHASE_MAX_PLANE": "0"}, [("gone", r"st27_pair_phase_kernel"), ("absent", r"st27_phase_kernel"), ("new", r"st27_color_sweep_kernel")]),
    "st27_pair_0_plane_all": ({"PMG_ST27_PAIR": "0", "PMG_ST27_PHASE_MAX_PLANE": "1000000000"}, [("gone", r"st27_pair_phase_kernel"), ("new", r"st27_phase_kernel"), ("absent", r"st27_color_sweep_kernel")]),
    "st27_pack_remainder_0": ({"PMG_ST27_PACK_REMAINDER": "0"}, [("gone", r"st27_pair_phase_kernel<\w+, \w+, \w+, \w+, true>"), ("gone", r"st27_pair_residual_kernel<true>")]),
    "transfer_generic": ({"PMG_TRANSFER_GENERIC": "1"}, [("gone", r"st27_restrict_full_kernel"), ("gone", r"q1_prolong_add_quad_kernel")]),
    "mg_prolong_both": ({"PMG_MG_PROLONG_BOTH": "1"}, [("launches", r"q1_prolong_add")]),
    "mg_no_stencil": ({"PMG_MG_NO_STENCIL": "1"}, [("gone", r"st27_pair_phase_kernel"), ("gone", r"st27_restrict")]),
    "mg_csr_transfers": ({"PMG_MG_CSR_TRANSFERS": "1"}, [("gone", r"q1_restrict"), ("gone", r"q1_prolong_add"), ("gone", r"grid_residual_restrict_kernel"), ("gone", r"st27_restrict")]),
    "sell_locality_0": ({"PMG_SELL_LOCALITY": "0"}, [("meta", "meta/layout/config4")]),
    "sell_locality_2": ({"PMG_SELL_LOCALITY": "2"}, [("meta", "meta/layout/lap99x99")]),
    "mg_fused_zero_0": ({"PMG_MG_FUSED_ZERO": "0"}, [("launches", r"fill_zero_kernel")]),
}

def _config4_npz(path):
    from parmgmc_amd.unstructured import assemble_p1, build_hierarchy, read_gmsh41_triangles, refine_uniform

    xy, tris = read_gmsh41_triangles(HERE / "golden" / "lshape.msh")
    for _ in range(5):
        xy, tris = refine_uniform(xy, tris)
    ops, ps = build_hierarchy(assemble_p1(xy, tris, 1.0), coarse_max=2000)
    arrays = {"nlevels": np.array(len(ops))}
    for l, (rp, ci, v) in enumerate(ops):
        arrays.update({f"rp{l}": rp, f"ci{l}": ci, f"v{l}": v})
    for l in range(1, len(ops)):
        rp, ci, v = ps[l]
        arrays.update({f"prp{l}": rp, f"pci{l}": ci, f"pv{l}": v})
    np.savez(path, **arrays)


def read_kernel_trace(d):
    """(kernel name, grid size) of every dispatch in a rocprofv3 --kernel-trace csv under d"""
    files = sorted(Path(d).rglob("*kernel_trace.csv"))
    assert files, f"rocprofv3 wrote no kernel_trace.csv under {d}"
    out = set()
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                out.add((row["Kernel_Name"], (int(row["Grid_Size_X"]), int(row["Grid_Size_Y"]), int(row["Grid_Size_Z"]))))
    return out


def _compare(res, ref):
    """keys of ref whose results differ from res in a single byte (dtype and shape included); meta prefixes that differ"""
    keys = sorted(k for k in ref if not k.startswith("meta/"))
    assert sorted(k for k in res if not k.startswith("meta/")) == keys
    differ = [k for k in keys if res[k].dtype != ref[k].dtype or res[k].shape != ref[k].shape or res[k].tobytes() != ref[k].tobytes()]
    meta = {k for k in ref if k.startswith("meta/") and res[k].tobytes() != ref[k].tobytes()}
    return differ, meta


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """config name -> (result keys that differ from the default child's, meta keys that differ, kernel launches or None).
    The children run one at a time; the first one that fails, is killed or times out stops the fixture."""
    tmp = tmp_path_factory.mktemp("switches")
    cfg4 = tmp / "config4.npz"
    _config4_npz(cfg4)
    prof = shutil.which("rocprofv3")
    base = {k: v for k, v in os.environ.items() if not k.startswith("PMG_") or k == "PMG_LIBRARY"}
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    done, error, ref = {}, None, None
    for name, (env, _) in CONFIGS.items():
        out, tdir = tmp / f"{name}.npz", tmp / f"trace_{name}"
        cmd = py + [str(CHILD), str(out), str(cfg4)]
        if prof:
            cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", str(tdir), "--"] + cmd
        try:
            p = subprocess.run(cmd, env=dict(base, **env), cwd=str(HERE.parent), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
            error = f"child {name} ({env}) timed out after {CHILD_TIMEOUT} s; stderr:\n{err[-4000:]}"
            break
        if p.returncode != 0 or not out.exists():
            error = f"child {name} ({env}) exited with {p.returncode}; stderr:\n{p.stderr[-4000:]}"
            break
        with np.load(out) as z:
            res = {k: z[k] for k in z.files}
        out.unlink()
        if ref is None:
            ref = res
        done[name] = _compare(res, ref) + (read_kernel_trace(tdir) if prof else None,)
        if prof:
            shutil.rmtree(tdir)
    return done, error


def _get(runs, name):
    done, error = runs
    for n in ("default", name):
        if n not in done:
            pytest.fail(error or f"child {n} did not run")
    return done[name], done["default"]


@pytest.mark.parametrize("name", [c for c in CONFIGS if c != "default"])
def test_switch_gives_the_default_bits(runs, name):
    (differ, _, _), _ = _get(runs, name)
    assert not differ, f"{name}: not bit-identical to the defaults on {differ}"


def _matching(launches, pattern):
    rx = re.compile(pattern)
    return {(k, g) for k, g in launches if rx.search(k)}


@pytest.mark.parametrize("name", [c for c in CONFIGS if c != "default"])
def test_switch_reaches_its_kernels(runs, name):
    (_, meta, launches), (_, _, ref_launches) = _get(runs, name)
    if launches is not None:  # what the switch changed, for the record (pytest -rP)
        names = lambda ls: {re.sub(r"^void |\(anonymous namespace\)::|\(.*", "", k) for k, _ in ls}
        print(f"{name}: gone {sorted(names(ref_launches) - names(launches))}, new {sorted(names(launches) - names(ref_launches))}, "
              f"launch shapes changed for {sorted(names(ref_launches ^ launches))}")
    for kind, pat in CONFIGS[name][1]:
        if kind == "meta":
            assert any(k.startswith(pat) for k in meta), f"{name}: {pat} unchanged"
            continue
        if launches is None:
            continue  # no rocprofv3: the bit comparison still ran
        mine, dflt = _matching(launches, pat), _matching(ref_launches, pat)
        if kind == "gone":
            assert dflt and not mine, f"{name}: {pat} should run by default ({len(dflt)}) and not here ({len(mine)})"
        elif kind == "new":
            assert mine and not dflt, f"{name}: {pat} should run here ({len(mine)}) and not by default ({len(dflt)})"
        elif kind == "absent":
            assert not mine, f"{name}: {pat} ran: {sorted(mine)[:3]}"
        else:
            assert mine and dflt and mine != dflt, f"{name}: launches of {pat} unchanged"
    if launches is None:
        pytest.skip("rocprofv3 not on PATH: kernel liveness not checked (the meta facts and the bits were)")


@pytest.mark.parametrize("shape", list(SHAPE_BRANCHES), ids=lambda s: "x".join(map(str, s)))
def test_shape_reaches_its_grid_mapping(runs, shape):
    """the restatement of the host's mapping gives the table's branch, and the default child launched exactly that sweep"""
    m = sweep_mapping(*shape)
    flags, gsize = m.flags, m.gsize
    assert flags == SHAPE_BRANCHES[shape]
    (_, _, launches), _ = _get(runs, "default")
    if launches is None:
        pytest.skip("rocprofv3 not on PATH")
    pat = SWEEP_TAIL if flags["tail"] else (SWEEP_PACKED if flags["packed"] else SWEEP_PLAIN)
    assert any(g == gsize for _, g in _matching(launches, pat)), f"no {pat} launch of grid {gsize}"


def test_halo_kernel_runs_on_the_plain_unpacked_mapping(runs):
    """the loopback workload of the child launched the in-kernel halo kernel one line per wavefront (not packed, no tail), with
    the grid the halo rule gives: XCD bands of ceil(ny / 8) lines, sentinel lines behind a short last band"""
    m = sweep_mapping(*HALO_TRACE_SHAPE, halo=True)
    assert not m.packed and not m.tail and m.banded and m.gsize == HALO_TRACE_GSIZE
    (_, _, launches), _ = _get(runs, "default")
    if launches is None:
        pytest.skip("rocprofv3 not on PATH")
    assert any(g == m.gsize for _, g in _matching(launches, SWEEP_HALO_PLAIN)), f"no {SWEEP_HALO_PLAIN} launch of grid {m.gsize}"
