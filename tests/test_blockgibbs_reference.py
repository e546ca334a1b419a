"""The plain numpy block Gibbs reference of tests/blockgibbs_cases.py, on its own (CPU): its sweep maps have A^-1 as their
stationary covariance, forward and symmetric, with overlapping (vertex-star) and disjoint (cell, line) blocks; and the stated
first-fit rule gives a valid block colouring.  The GPU tests compare the device with this reference."""
import numpy as np
import pytest

import oracle as O
from blockgibbs_cases import FWD, SYM, Reference, cell_blocks, colors_valid, conflicts, covariance_error, first_fit_colors, line_blocks, ref_maps, squared, star_blocks


def _cases():
    e5, e05 = O.ex6_matrix(9, 0.5), O.ex6_matrix(9, 0.05)
    out = []
    for name, A, pat in (("ex6sq", squared(e5), e5), ("ex6", e05, e05)):
        out += [(f"{name}-stars", A, star_blocks(pat)), (f"{name}-cells", A, cell_blocks(9, 9)), (f"{name}-lines", A, line_blocks(9, 9))]
    L3 = O.shifted_laplace(5, 4, 3, 2.0)
    out.append(("lap3d-stars", L3, star_blocks(L3)))
    return out


CASES = _cases()
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("name,A,blocks", CASES, ids=IDS)
def test_first_fit_colouring_is_valid_and_is_the_stated_rule(name, A, blocks):
    col = first_fit_colors(A, blocks)
    assert colors_valid(A, blocks, col)
    nb = conflicts(A, blocks)
    for p in range(len(blocks)):  # first-fit: every smaller colour is taken by an EARLIER conflicting block
        earlier = {int(col[q]) for q in nb[p] if q < p}
        assert col[p] not in earlier and set(range(col[p])) <= earlier, p
    bad = col.copy()
    q = next(iter(nb[0]))
    bad[0] = bad[q]
    assert not colors_valid(A, blocks, bad)  # the check sees one clash


@pytest.mark.parametrize("sweep", [FWD, SYM], ids=["forward", "symmetric"])
@pytest.mark.parametrize("name,A,blocks", CASES, ids=IDS)
def test_reference_sweep_maps_have_the_target_covariance(name, A, blocks, sweep):
    R = Reference(A, blocks)
    G, N = ref_maps(R, first_fit_colors(A, blocks), sweep)
    rho = float(np.abs(np.linalg.eigvals(G)).max())
    err = covariance_error(A, G, N)
    print(f"{name} sweep {sweep}: spectral radius {rho:.3f}, covariance error {err:.2e}")
    assert rho < 1.0
    assert err <= 1e-10
