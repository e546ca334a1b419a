"""The shape tables of grid_mappings.py against the restated mapping rule, without a GPU: every shape reaches the branch
its table declares under the single-device rule and under the halo rule, and the tables together cover what their users'
docstrings claim.  Moving a shape back to a line length that packs (nx = 12, say) fails here."""
import pytest

import grid_mappings as M
from grid_mappings import sweep_mapping

CASES = [(name, shape) for name, table in M.TABLES.items() for shape in table]


@pytest.mark.parametrize("name,shape", CASES, ids=[f"{n}-" + "x".join(map(str, s)) for n, s in CASES])
def test_tabled_shape_reaches_its_declared_branch(name, shape):
    single, halo = M.TABLES[name][shape]
    nx, ny, nz = shape[:3]
    assert sweep_mapping(nx, ny, nz).flags == single
    assert sweep_mapping(nx, ny, nz, halo=True).flags == halo
    assert not halo["tail"] and not halo["flat"]
    assert nz <= 9 and nx * ny * nz <= 3.1e5  # the suite's grids stay small


def test_trace_table_states_the_single_device_rule():
    for shape, flags in M.SHAPE_BRANCHES.items():
        assert sweep_mapping(*shape).flags == flags, shape
    for shape in [(170, 62, 3), (170, 64, 3), (400, 62, 3), (255, 65, 3)]:  # the plain unpacked mapping, with and without bands / flat
        assert not M.SHAPE_BRANCHES[shape]["tail"] and not M.SHAPE_BRANCHES[shape]["packed"]
    m = sweep_mapping(*M.HALO_TRACE_SHAPE, halo=True)
    assert m.flags == M.BANDED and m.gsize == M.HALO_TRACE_GSIZE


def test_flat_shapes_cover_every_band_remainder():
    flat = [s for s, (single, _) in M.BAND_SHAPES.items() if single["flat"]]
    assert {sweep_mapping(*s).remainder for s in flat} == set(range(8))
    plain_flat = [s for s in flat if not M.BAND_SHAPES[s][0]["tail"]]
    assert {sweep_mapping(*s).remainder for s in plain_flat} == set(range(8))  # ... without the help of the tail mapping
    assert {61, 62, 63} <= {s[1] for s in plain_flat}
    for ny in (61, 62, 63):  # bands of 7 lines, five to seven of them with one line more
        m = sweep_mapping(170, ny, 5)
        assert m.bandw == 7 and m.remainder == ny - 56
    assert all(single == M.PACKED for single, _ in M.BAND_CONTROLS.values())
    assert {s[1] for s in M.BAND_CONTROLS} <= {s[1] for s in M.BAND_SHAPES}  # controls: line counts the band shapes run, too


def test_single_device_tables_hold_every_unpacked_branch():
    got = [sweep_mapping(*s) for s in M.UNPACKED_SHAPES]
    assert any(not (m.tail or m.packed or m.banded) for m in got)                  # plain
    assert any(m.banded and not m.flat and not m.tail for m in got)                # banded, whole line tiles
    assert any(m.flat and not m.tail and m.waves == 2 for m in got)                # flat, two wavefronts per line
    assert any(m.flat and m.tail for m in got)                                     # tail + flat
    slab = [sweep_mapping(*s) for s in M.SLAB_SHAPES]
    assert any(m.tail and not m.banded and s[0] % 256 == 1 for m, s in zip(slab, M.SLAB_SHAPES))  # the compact tail (nx = 4 tmain + 1)
    assert any(m.tail and not m.banded and s[0] % 256 != 1 for m, s in zip(slab, M.SLAB_SHAPES))  # several tail threads per line
    assert any(m.tail and m.flat for m in slab) and any(m.flat and not m.tail for m in slab)
    assert any(m.banded and not m.flat for m in slab) and any(m.waves == 2 for m in slab)
    for cuts in M.SLAB_CUTS:
        assert cuts[0] == 0 and cuts[-1] == 6 and cuts == sorted(cuts)
    starts = [lo for cuts in M.SLAB_CUTS for lo in cuts[1:-1]]
    assert any(lo & 1 for lo in starts) and any(not lo & 1 for lo in starts)       # odd and even kz0
    assert any(hi - lo == 1 for cuts in M.SLAB_CUTS for lo, hi in zip(cuts, cuts[1:]))  # a one-plane slab


def _halo_kinds(shapes):
    got = {s: sweep_mapping(*s[:3], halo=True) for s in shapes}
    return {
        "unpacked plain": [s for s, m in got.items() if not m.packed and not m.banded],
        "banded, whole line tiles": [s for s, m in got.items() if m.banded and m.bandw % 4 == 0 and 8 * m.bandw == s[1]],
        "banded, short last band": [s for s, m in got.items() if m.banded and 8 * m.bandw > s[1]],
        "banded, band width no multiple of 4": [s for s, m in got.items() if m.banded and m.bandw % 4],
        "three wavefronts per line": [s for s, m in got.items() if m.waves == 3],
        "one-plane slab": [s for s, m in got.items() if not m.packed and s[2] == 1],
        "packed control": [s for s, m in got.items() if m.packed],
    }


def test_halo_table_holds_every_kind_of_launch():
    for kind, shapes in _halo_kinds(M.HALO_SHAPES).items():
        assert shapes, f"no halo shape is {kind}"


def test_rank_and_vcycle_halo_shapes_are_unpacked():
    for table in (M.HALO_RANK_SHAPES, M.HALO_VCYCLE_SHAPES):
        for s in table:
            assert not sweep_mapping(*s[:3], halo=True).packed, s
    kinds = _halo_kinds(list(M.HALO_RANK_SHAPES) + list(M.HALO_VCYCLE_SHAPES))
    for kind in ("unpacked plain", "banded, short last band", "banded, band width no multiple of 4", "three wavefronts per line"):
        assert kinds[kind], kind
    from parmgmc_amd.slab import slab_cuts

    sizes = {s: [hi - lo for lo, hi in zip(slab_cuts(s[2], s[3]), slab_cuts(s[2], s[3])[1:])] for s in M.HALO_RANK_SHAPES}
    assert sizes[(170, 61, 6, 5)] == [2, 1, 1, 1, 1]
    assert any(1 in v for v in sizes.values()) and any(min(v) >= 2 for v in sizes.values())
