"""The shape table of st27_splits.py against the restated rule, and the restated rule's constants against the .hip sources,
without a GPU: every class-stencil shape reaches the branch of split_pairs it declares, for the sweep and for the residual, the
table as a whole covers every branch, both sides of each pack threshold, every line count modulo 8 and both sides of the
plane-kernel rule -- and none of that was covered by the extents the suite ran before (line lengths of 2^k + 1 points and 144,
line counts of at most 5 or 8 m + 1).  Moving a tabled extent back to such a value fails here."""
import re
from pathlib import Path

import pytest

import st27_splits as M

CSRC = Path(__file__).resolve().parent.parent / "parmgmc_amd" / "csrc"
SHAPES = list(M.SHAPES)
IDS = ["x".join(map(str, s)) for s in SHAPES]
SV, SH = M.SWEEP
RV, RH = M.RESID


def test_restated_constants_are_the_kernels():
    pair = (CSRC / "kernels_stencil27_pair.hip").read_text()
    const = lambda name: int(re.search(r"constexpr int %s\s*=\s*(\d+);" % name, pair).group(1))  # noqa: E731
    assert (const("PT"), const("VALID"), const("HL")) == (M.PT, SV, SH)
    assert SV + 2 * SH == 64 and RV + 2 * RH == 64  # a wavefront: the valid pairs and the halo lanes on both sides
    # the sweep's launches: tiles of 2 PT lines, PT + 1 wavefronts, split_pairs(npairs, VALID, HL)
    assert "split_pairs(npairs, VALID, HL)" in pair and "(S.ny + 2 * PT - 1) / (2 * PT)" in pair and "block(64, PT + 1)" in pair
    assert "nbyp = (nby + P.nseg - 1) / P.nseg" in pair
    # the residual's: 62 valid pairs, one halo lane, tiles of 4 lines
    res = pair[pair.index('extern "C" int pmgk_st27_residual_pair'):]
    m = re.search(r"split_pairs\(npairs, (\d+), (\d+)\)", res)
    assert (int(m.group(1)), int(m.group(2))) == (RV, RH)
    assert f"p     = {RV} * bx - {RH} + lane" in pair and f"inner = lane >= {RH} && lane <= {RV}" in pair
    assert "(S->ny + 3) / 4" in res and "(S->ny + 4 * P.nseg - 1) / (4 * P.nseg)" in res and res.count("dim3(64, 4)") == 2 and M.RESID_TILE == 4
    # split_pairs and xcd_grid themselves
    assert "nbx = (npairs + valid - 1) / valid, rem = npairs - valid * (nbx - 1), segw = rem + 2 * halo" in pair
    assert "if (env && 64 / segw >= 2)" in pair and "P.nseg     = 64 / segw" in pair
    assert "return (unsigned)(8 * nbx * ((T + 7) / 8));" in pair
    plane = (CSRC / "kernels_stencil27.hip").read_text()
    assert int(re.search(r'\{"PMG_ST27_PHASE_MAX_PLANE", INT, (\d+), PROCESS\}', (CSRC / "pmg_switch.c").read_text()).group(1)) == M.PLANE_LIMIT  # the default: its row of the switch table
    assert "plane_limit = pmg_switch(PMG_SW_ST27_PHASE_MAX_PLANE);" in plane
    assert "(int64_t)S->nx * S->ny <= plane_limit" in plane and "dim3(cz), dim3(1024)" in plane


def test_restated_split_on_the_lines_the_suite_ran_before():
    """the splits of the line lengths the suite reached before this table, as its issue computed them"""
    both = lambda nx: (M.sweep_split(nx), M.residual_split(nx))  # noqa: E731
    for nx in (2, 3, 5, 9, 17, 33):
        assert all(M.kind(P, v) == "all packed" for P, v in zip(both(nx), (SV, RV)))
    assert [M.kind(P, v) for P, v in zip(both(65), (SV, RV))] == ["one partial", "one partial"]
    got = {nx: [(P.nbx_main, P.segw, P.nseg) for P in both(nx)] for nx in (129, 144, 257)}
    assert got == {129: [(1, 9, 7), (1, 5, 12)], 144: [(1, 16, 4), (1, 12, 5)], 257: [(2, 13, 4), (2, 7, 9)]}
    assert M.xcd_grid(2, 33, 129) == 8 * 2 * 533 and M.xcd_grid(1, 1, 1) == 8


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_tabled_shape_reaches_its_declared_branch(shape):
    sweep, resid, why = M.SHAPES[shape]
    cx, cy, cz = shape
    assert M.kind(M.sweep_split(cx), SV) == sweep and M.kind(M.residual_split(cx), RV) == resid
    assert cx not in M.SUITE_NX, "a line length the suite ran before"
    assert cz == 1 or all(p > 0 for p in M.phase_planes(cz))
    assert why
    # without packing every remainder is a segment of the one-line-per-wavefront launch
    assert not M.sweep_split(cx, pack=False).packed and M.sweep_split(cx, pack=False).nbx_main == ((cx + 1) // 2 + SV - 1) // SV


def test_what_single_shapes_are_there_for():
    s, r = M.sweep_split, M.residual_split
    assert tuple(s(55))[2:] == (32, 2, 28) and tuple(r(55))[2:4] == (30, 2)
    assert not s(57).packed and s(57).rem == 29 and r(57).segw == 31
    assert r(59).segw == 32 and r(59).nseg == 2 and M.phase_planes(1) == [1, 0]
    assert not r(61).packed and r(61).rem == 31 and 1024 < 61 * 18 <= M.PLANE_LIMIT
    assert s(119).rem == SV and s(120).rem == SV and 119 % 2 == 1 and 120 % 2 == 0
    assert tuple(s(121)) == (1, 60, 5, 12, 1) and M.sweep_idle_segments(121, 17) == 9 and r(121).rem == 61
    assert r(123).rem == RV and r(123).nbx_main == 1
    assert tuple(r(125)) == (1, 62, 3, 21, 1) and 12 % 8 == 4
    assert tuple(s(175)) == (1, 60, 32, 2, 28)
    assert tuple(s(177))[:2] == (2, -1) and s(177).rem == 29
    assert s(199).rem == 40 and r(199).rem == 38 and not s(199).packed and not r(199).packed
    assert s(239).nbx_main == 2 and s(239).rem == SV
    assert tuple(s(241)) == (2, 120, 5, 12, 1)
    assert r(247).nbx_main == 2 and r(247).rem == RV


@pytest.mark.parametrize("name,split,valid,halo", [("sweep", M.sweep_split, SV, SH), ("residual", M.residual_split, RV, RH)])
def test_table_covers_every_branch_of_the_split(name, split, valid, halo):
    P = {s: split(s[0]) for s in SHAPES}
    kinds = {M.kind(p, valid) for p in P.values()}
    assert kinds == {"all packed", "one partial", "one full", "packed behind main", "unpacked behind main", "full segments"}
    assert any(p.nbx_main >= 2 for p in P.values())
    widest = 32 - 2 * halo  # the widest remainder that packs: two segments of 32 lanes
    for nmain in (0, 1):  # both sides of the threshold, with and without a main segment in front
        rems = {p.rem: p.packed for p in P.values() if (p.nbx_main - (0 if p.packed else 1)) == nmain}
        assert rems.get(widest) is True and rems.get(widest + 1) is False, (name, nmain, rems)
    assert any(p.packed and p.nseg == 2 for p in P.values())
    assert any(p.packed and p.rem == 1 and p.nbx_main >= 1 for p in P.values())  # a remainder of one pair behind a main segment
    assert any(p.packed and p.rem == 1 and p.nbx_main >= 2 for p in P.values()) or name == "residual"
    idle = M.sweep_idle_segments if name == "sweep" else M.residual_idle_lines
    assert any(idle(cx, cy) > 0 for cx, cy, _ in SHAPES) and any(P[s].packed and idle(*s[:2]) == 0 for s in SHAPES)
    # ... and none of it by the line lengths the suite ran before
    old = [split(nx) for nx in M.SUITE_NX]
    assert {M.kind(p, valid) for p in old} == {"all packed", "one partial", "packed behind main"}
    assert not any(p.rem in (widest, widest + 1, valid) for p in old)
    assert not any(p.packed and p.nseg == 2 for p in old)
    assert not any(p.packed and p.rem == 1 and p.nbx_main for p in old)


def test_table_covers_line_counts_planes_and_the_plane_rule():
    assert {cy % 8 for _, cy, _ in SHAPES if cy > 5} == set(range(8))  # every residue, beyond the five lines the suite had
    assert {cy % 8 for _, cy, _ in SHAPES} == set(range(8))
    new = [cy for _, cy, _ in SHAPES if not M.suite_ny_before(cy)]
    assert {cy % 8 for cy in new} == {0, 2, 3, 4, 5, 6, 7}
    assert {cz for _, _, cz in SHAPES} == {1, 2, 3, 4}
    # a backward sweep starts its first stage on line -1 in every tile position; stage lines past the plane's end: a last tile
    # with 1 .. 8 lines
    assert {(cy - 1) % 8 + 1 for _, cy, _ in SHAPES} == set(range(1, 9))
    planes = [cx * cy for cx, cy, _ in SHAPES]
    assert any(p <= M.PLANE_LIMIT for p in planes) and any(p > M.PLANE_LIMIT for p in planes)
    assert any(1024 < p <= M.PLANE_LIMIT for p in planes)  # the plane kernel's 1024 threads stride over the plane
    assert any(M.plane_kernel(cx, cy) for cx, cy, _ in SHAPES) and not all(M.plane_kernel(cx, cy) for cx, cy, _ in SHAPES)


def test_hierarchies_beside_the_table():
    (g3, l3), (g2, l2), (gq, lq) = M.THREE_LEVEL, M.SEMICOARSENED, M.FLAT_QUAD
    assert M.st27_levels(g3, l3, True) == [(241, 17, 5), (121, 9, 3)] and M.st27_levels(g3, l3, False) == [(241, 17, 5)]
    assert M.st27_levels(g2, l2, True) == [(121, 17, 1)]
    assert M.coarsen(gq) == (257, 129, 2) and M.quad_prolong_blocks(*gq[:2]) == (66, 72)  # >= 64 blocks: XCD runs, padded to 8 m
    tabled_cx = {s[0] for s in M.SHAPES}
    for (grid, levels), first in zip(M.VCYCLE_SHAPES.items(), M.VCYCLE_LEVELS):
        assert M.st27_levels(grid, levels, False) == [first] and first[0] in tabled_cx and levels == 3
        assert all(d % 2 == 1 for d in first)  # only a level of 2 c - 1 points coarsens again
        cx, cy, cz = M.st27_levels(grid, levels, True)[-1]
        assert cx * cy * cz <= 1200  # the dense Cholesky level stays small
    assert {M.kind(M.sweep_split(s[0]), SV) for s in M.VCYCLE_LEVELS} == {"one partial", "packed behind main", "unpacked behind main"}
    assert {s[0] for s in M.VCYCLE_LEVELS} == {57, 121, 177, 199}
