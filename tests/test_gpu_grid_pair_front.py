"""The row addressing of grid_color_pair_sweep_kernel -- one scalar base per array (row j of plane k0 - 1) and a wave-uniform
unsigned 32-bit byte offset per row, the clamps at the faces selecting between offsets -- at the smallest shapes at which it
can go wrong (pair_front_workloads.py): one and two x blocks, ny = 1, 2, 8, 9, nz = 2 .. 5, plane ranges of nz = 5 and a slab
with kz0 > 0.  Three noisy sweeps at omega = 1, both colours:

  * the default build against PMG_GRID_PLANE_PAIR=0 (the one-plane kernel), each in a fresh child process: bit for bit;
  * against the oracle to 1e-13 of max|y|: whole chains against gibbs_samples, plane ranges against a restatement of one
    colour pass over a range of planes in numpy, which is itself held to gibbs_samples on whole chains;
  * a control on the reference side: the restatement with a WRONG offset on a face row -- the lower face reads the clamped
    row with the coefficient of a neighbour -- must be noticed by the same comparison.

With rocprofv3 on PATH the default child runs under its kernel trace and every noisy sweep must be a plane-pair launch."""
import csv
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle as O
import pair_front_workloads as W

HERE = Path(__file__).resolve().parent
CHILD = HERE / "pair_front_workloads.py"
CHILD_TIMEOUT = 180  # s; a child takes seconds beyond the start of torch
TOL = 1e-13
PAIR = r"grid_color_pair_sweep_kernel<\w+>"
ONE_NOISY = r"grid_color_sweep_kernel<true, "


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """pair on -> (results, kernel names or None)"""
    tmp = tmp_path_factory.mktemp("pair_front")
    prof = shutil.which("rocprofv3")
    base = {k: v for k, v in os.environ.items() if not k.startswith("PMG_") or k == "PMG_LIBRARY"}
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    done = {}
    for on in (False, True):
        out, tdir = tmp / f"front_{int(on)}.npz", tmp / f"trace_{int(on)}"
        cmd = py + [str(CHILD), str(out)]
        if prof and on:
            cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", str(tdir), "--"] + cmd
        env = dict(base, **({} if on else {"PMG_GRID_PLANE_PAIR": "0"}))
        p = subprocess.run(cmd, env=env, cwd=str(HERE.parent), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        if p.returncode != 0 or not out.exists():
            pytest.fail(f"child (pair {'on' if on else 'off'}) exited with {p.returncode}; stderr:\n{p.stderr[-4000:]}")
        with np.load(out) as z:
            res = {k: z[k] for k in z.files}
        names = None
        if prof and on:
            files = sorted(tdir.rglob("*kernel_trace.csv"))
            assert files, f"rocprofv3 wrote no kernel_trace.csv under {tdir}"
            names = set()
            for f in files:
                with open(f, newline="") as fh:
                    names |= {row["Kernel_Name"] for row in csv.DictReader(fh)}
            shutil.rmtree(tdir)
        done[on] = (res, names)
    return done


class Reference:
    """One colour pass of the noisy omega = 1 sweep over a range of planes, on (nzg, ny, nx) arrays: y <- (w + h2 * sum of
    the in-domain neighbours) / d on the points of colour c of the planes, w = xi * sqrtdiag + b from the oracle's noise and
    tables.  wrong_face: the lower face reads the clamped row (itself) with coefficient h2 instead of 0."""

    def __init__(self, nx, ny, nzg, b, wrong_face=False):
        self.shape, self.b, self.wrong = (nzg, ny, nx), b, wrong_face
        self.A = O.shifted_laplace(nx, ny, nzg, W.KAPPA)
        m = self.A.scipy()
        self.d = m.diagonal().reshape(self.shape)
        self.h2 = -m[0, 1]
        self.sd = O.sqrtdiag(self.A, 1.0, True)
        k, j, i = np.meshgrid(np.arange(nzg), np.arange(ny), np.arange(nx), indexing="ij")
        self.colour, self.k = (i + j + k) & 1, k

    def colour_pass(self, y, c, k0, k1, counter):
        nzg, ny, nx = self.shape
        w = O.prepare_rhs(O.noise_grid(nx, ny, nzg, W.SEED, counter), self.sd, self.b).reshape(self.shape)
        Y = y.reshape(self.shape)
        P = np.pad(Y, 1)
        if self.wrong:
            P[0, 1:-1, 1:-1] = Y[0]
        s = P[:-2, 1:-1, 1:-1] + P[2:, 1:-1, 1:-1] + P[1:-1, :-2, 1:-1] + P[1:-1, 2:, 1:-1] + P[1:-1, 1:-1, :-2] + P[1:-1, 1:-1, 2:]
        new = (w + self.h2 * s) / self.d
        mask = (self.colour == c) & (self.k >= k0) & (self.k < k1)
        Y[mask] = new[mask]

    def chain(self, y0):
        y = y0.copy()
        for d in range(W.SWEEPS):
            for c in (0, 1):
                self.colour_pass(y, c, 0, self.shape[0], W.COUNTER0 + d)
        return y


def rel_err(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


@pytest.mark.gpu
def test_the_short_front_gives_the_one_plane_bits(runs):
    (ref, _), (res, names) = runs[False], runs[True]
    assert sorted(res) == sorted(ref) and len(ref) == len(W.SHAPES) + len(W.RANGE_SHAPES) * len(W.RANGES) + len(W.SLAB_RANGES)
    differ = [k for k in sorted(ref) if not np.array_equal(res[k].view(np.uint64), ref[k].view(np.uint64))]
    assert not differ, f"{len(differ)} of {len(ref)} vectors differ from the one-plane kernel's, first {differ[:5]}"
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in ref.values())
    if names is not None:  # every noisy sweep of the default child was a plane-pair launch
        assert any(re.search(PAIR, n) for n in names), sorted(names)
        assert not [n for n in names if re.search(ONE_NOISY, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("nx", [256, 512])
def test_whole_chains_match_the_oracle(runs, nx):
    res = runs[True][0]
    for shape in [s for s in W.SHAPES if s[0] == nx]:
        _, ny, nz = shape
        b, y0 = W.inputs(*shape)
        want = O.gibbs_samples(O.shifted_laplace(*shape, W.KAPPA), O.coloring_redblack(*shape), b, y0, W.SWEEPS, lambda d: O.noise_grid(nx, ny, nz, W.SEED, W.COUNTER0 + d), 1.0, O.SOR_FORWARD, True)
        err = rel_err(res[f"chain/{nx}x{ny}x{nz}"], want)
        print(shape, "chain", err)
        assert err < TOL, (shape, err)


def test_the_restatement_of_a_colour_pass_is_the_oracle_s():
    """what the plane ranges and the control are measured with, against gibbs_samples on whole chains (no GPU)"""
    for shape in W.RANGE_SHAPES + [(256, 1, 2)]:
        nx, ny, nz = shape
        b, y0 = W.inputs(*shape)
        want = O.gibbs_samples(O.shifted_laplace(*shape, W.KAPPA), O.coloring_redblack(*shape), b, y0, W.SWEEPS, lambda d: O.noise_grid(nx, ny, nz, W.SEED, W.COUNTER0 + d), 1.0, O.SOR_FORWARD, True)
        assert rel_err(Reference(nx, ny, nz, b).chain(y0), want) < TOL, shape


@pytest.mark.gpu
def test_plane_ranges_and_a_slab_match_the_oracle(runs):
    res = runs[True][0]
    for shape in W.RANGE_SHAPES:
        nx, ny, nz = shape
        b, y0 = W.inputs(*shape)
        R, y = Reference(nx, ny, nz, b), y0.copy()
        for kbegin, kcount, ctr in W.RANGES:
            for c in (0, 1):
                R.colour_pass(y, c, kbegin, kbegin + kcount, ctr)
            err = rel_err(res[f"range/{nx}x{ny}x{nz}/k{kbegin}+{kcount}"], y)
            print(shape, kbegin, kcount, err)
            assert err < TOL, (shape, kbegin, kcount, err)
        assert not np.array_equal(y, y0)
    nx, ny, nzg, kz0, nzo = W.SLAB
    b, y0 = W.inputs(nx, ny, nzg)
    R, y, own = Reference(nx, ny, nzg, b), y0.copy(), slice(kz0 * nx * ny, (kz0 + nzo) * nx * ny)
    for kbegin, kcount, ctr in W.SLAB_RANGES:
        for c in (0, 1):
            R.colour_pass(y, c, kz0 + kbegin, kz0 + kbegin + kcount, ctr)
        err = rel_err(res[f"slab/k{kbegin}+{kcount}"], y[own])
        print("slab", kbegin, kcount, err)
        assert err < TOL, (kbegin, kcount, err)
    assert np.array_equal(y[: kz0 * nx * ny], y0[: kz0 * nx * ny])  # the plane below the slab is only read


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(256, 1, 2), (512, 9, 5)], ids=lambda s: "x".join(map(str, s)))
def test_a_wrong_offset_on_a_face_row_is_noticed(runs, shape):
    """control: the reference with the lower face's down row read from the clamped address WITH a coefficient"""
    nx, ny, nz = shape
    b, y0 = W.inputs(*shape)
    got = runs[True][0][f"chain/{nx}x{ny}x{nz}"]
    good, bad = rel_err(got, Reference(nx, ny, nz, b).chain(y0)), rel_err(got, Reference(nx, ny, nz, b, wrong_face=True).chain(y0))
    print(shape, good, bad)
    assert good < TOL < bad, (shape, good, bad)
