"""The whole geometric (DMDA) V-cycle against the oracle at the shapes where the host's kernel choices change: tail /
packed / banded + flat thread mappings of the grid level (which shape reaches which: SHAPE_BRANCHES of
grid_mappings.py, checked against the kernel trace in test_gpu_switches.py), class-stencil planes at the plane-kernel limit, wide
class-stencil lines with a packed x remainder, 2-D and semicoarsened levels (no fused residual + restriction, general
Q1 transfers), even extents on the coarsest levels and minimal extents -- under the settings that select the
one-colour prolongation (omega = 1: forward, backward and symmetric skip different colours) and those that do not.

The class-stencil levels of these shapes have lines of 2^k + 1 points (and 144) and at most 5 or 8 m + 1 lines; the other ways
a class-stencil line is cut into wavefronts (a full segment, an unpacked remainder behind one, both sides of the pack
threshold, a remainder of one pair) and the other positions of a plane's last line tile are the shapes of st27_splits.py
(SHAPES, VCYCLE_SHAPES), run kernel by kernel and as whole V-cycles in test_gpu_st27_splits.py.

Every sample of a 3-sample chain is compared, at the relative max-norm tolerance of test_gpu_mgmc.py (1e-11: Galerkin
entries and residual sums are taken in another order).  The negative control shifts one level's noise counter in the
oracle and requires the sampler to be far outside that tolerance: every level's contribution is visible."""
import functools

import numpy as np
import pytest

import oracle as O
from test_gpu_mgmc import dev, host, oracle_chain, oracle_hierarchy

pytestmark = pytest.mark.gpu
TOL = 1e-11
KAPPA = 1.5

SHAPES = [
    ((257, 9, 9), 3),      # tail mapping, 1 tail thread per line (65 threads per line)
    ((287, 5, 5), 2),      # tail mapping, 8 tail threads (72); coarse x extent 144 (even)
    ((257, 65, 9), 4),     # tail + XCD-banded + flat dispatch of the grid level
    ((65, 65, 65), 4),     # packed grid level; class-stencil planes of 33 x 33 = 1089 points (plane kernel limit 1100)
    ((129, 65, 17), 4),    # anisotropic; class-stencil lines of 65 points: packed x remainder (33 pairs = 31 + 2)
    ((257, 257, 1), 5),    # 2-D: z never coarsens -- semicoarsened Q1 transfers, no fused residual + restriction
    ((9, 9, 129), 4),      # x / y reach extent 2 (even) on the coarsest levels while z keeps coarsening
    ((33, 3, 33), 2),      # minimal y extent
    ((5, 5, 5), 2),        # minimal grid
    ((513, 9, 9), 3),      # tail mapping behind two full wavefronts per line; the single-device side of the distributed V-cycle
                           # whose slabs sweep it one line per wavefront under the halo hand-shake (test_gpu_dist_two_ranks.py)
]
IDS = ["x".join(map(str, g)) + f"-L{l}" for g, l in SHAPES]

# name -> (scaled, omega, sweep, nu, coarse, coarse its, correction form)
SETTINGS = {
    "default": (False, 1.0, O.SOR_FORWARD, 1, "cholsampler", 1, False),
    "backward_omega1": (False, 1.0, O.SOR_BACKWARD, 1, "cholsampler", 1, False),
    "symmetric_omega1": (False, 1.0, O.SOR_SYMMETRIC, 1, "cholsampler", 1, False),
    "symmetric_scaled_nu2_gibbs_correction": (True, 1.3, O.SOR_SYMMETRIC, 2, "gibbs", 2, True),
}


@functools.lru_cache(maxsize=None)
def hierarchy(grid, levels):
    return oracle_hierarchy(*grid, KAPPA, levels)


def inputs(grid):
    n = int(np.prod(grid))
    rng = np.random.default_rng(n)
    return rng.standard_normal(n), rng.standard_normal(n)


def run_sampler(grid, levels, setting, y0, its, guesszero, seed=0xC0DE, counter0=4):
    from parmgmc_amd import MGMC

    scaled, omega, sweep, nu, coarse, cits, literal = SETTINGS[setting]
    b, _ = inputs(grid)
    mg = MGMC(*grid, KAPPA, levels)
    mg.set_smoother(scaled, omega, sweep, nu)
    mg.set_coarse(coarse, cits)
    mg.set_correction_form(literal)
    mg.setup()
    seen = []
    yd = dev(y0)
    nxt = mg.sample(dev(b), yd, its, seed=seed, counter0=counter0, guesszero=guesszero, callback=lambda it, y: seen.append(host(y).copy()))
    assert nxt == counter0 + its
    assert np.array_equal(seen[-1], host(yd))
    mg.destroy()
    return seen


def run_oracle(grid, levels, setting, y0, its, guesszero, seed=0xC0DE, counter0=4, shift=None):
    scaled, omega, sweep, nu, coarse, cits, _ = SETTINGS[setting]
    b, _ = inputs(grid)
    return oracle_chain(grid, KAPPA, levels, b, y0, its, seed, counter0, guesszero, nu=nu, scaled=scaled, omega=omega, sweep=sweep,
                        coarse=coarse, coarse_its=cits, lv=hierarchy(grid, levels), shift=shift)


def rel_err(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("grid,levels", SHAPES, ids=IDS)
def test_vcycle_chain_matches_oracle(grid, levels, setting):
    _, y0 = inputs(grid)
    got = run_sampler(grid, levels, setting, y0, 3, False)
    want = run_oracle(grid, levels, setting, y0, 3, False)
    for it, (g, w) in enumerate(zip(got, want)):
        assert rel_err(g, w) < TOL, f"sample {it}: {rel_err(g, w):.3e}"


@pytest.mark.parametrize("grid,levels", SHAPES, ids=IDS)
def test_vcycle_chain_from_zero_guess_matches_oracle(grid, levels):
    n = int(np.prod(grid))
    got = run_sampler(grid, levels, "default", np.zeros(n), 3, True)
    want = run_oracle(grid, levels, "default", np.zeros(n), 3, True)
    for it, (g, w) in enumerate(zip(got, want)):
        assert rel_err(g, w) < TOL, f"sample {it}: {rel_err(g, w):.3e}"


@pytest.mark.parametrize("setting", ["default", "backward_omega1"])
@pytest.mark.parametrize("grid,levels", [((257, 65, 9), 4), ((129, 65, 17), 4), ((257, 257, 1), 5)], ids=["257x65x9-L4", "129x65x17-L4", "257x257x1-L5"])
def test_every_level_is_visible_above_the_tolerance(grid, levels, setting):
    """negative control: the oracle with one level's noise counter moved by one draw is not the sampler's chain"""
    _, y0 = inputs(grid)
    got = run_sampler(grid, levels, setting, y0, 2, False)
    assert rel_err(got[-1], run_oracle(grid, levels, setting, y0, 2, False)[-1]) < TOL
    for l in range(levels):
        w = run_oracle(grid, levels, setting, y0, 2, False, shift={l: 1})
        assert rel_err(got[0], w[0]) > 100 * TOL, f"level {l}: its noise does not show in the first sample"
