"""pmg_mcsor_setup refuses an automatic colouring that is not a distance-1 colouring of the stored pattern.  GREEDY, ITERATED and
LEXLEVELS only look at the columns a row lists; on a structurally non-symmetric pattern (r lists c, c does not list r) they can
give r and c one colour, and the sweep would then read y[c] while c is being updated.  The check runs on the host, before any
device call, so this is a CPU test."""
import numpy as np
import pytest

import oracle as O
from aij_workloads import one_sided
from parmgmc_amd import COLORING_GREEDY, COLORING_ITERATED, COLORING_LEXLEVELS, MCSOR, PMGError

RULES = [(COLORING_GREEDY, O.coloring_greedy), (COLORING_ITERATED, O.coloring_iterated), (COLORING_LEXLEVELS, O.coloring_lexlevels)]
IDS = ["greedy", "iterated", "lexlevels"]


def first_conflict(A, colors):
    """the first (r, c) in row-major storage order with r != c, colour(r) == colour(c)"""
    for r in range(A.n):
        for k in range(A.rowptr[r], A.rowptr[r + 1]):
            c = int(A.colidx[k])
            if c != r and colors[c] == colors[r]:
                return r, c
    return None


@pytest.mark.parametrize("rule,oracle_rule", RULES, ids=IDS)
def test_two_rows_one_sided(rule, oracle_rule):
    """row 0 lists column 1, row 1 lists only its diagonal: every automatic rule puts both rows into colour 0"""
    A = O.CSR(np.array([0, 2, 3]), np.array([0, 1, 1]), np.array([2.0, -1.0, 2.0]))
    assert list(oracle_rule(A)) == [0, 0]
    mc = MCSOR(A.rowptr, A.colidx, A.vals, rule)
    with pytest.raises(PMGError) as e:
        mc.setup()
    assert e.value.code == 62
    assert "rows 0 and 1 are coupled but share colour 0" in str(e.value)
    # nothing was set up: a second attempt fails the same way
    with pytest.raises(PMGError) as e:
        mc.setup()
    assert e.value.code == 62
    mc.destroy()


@pytest.mark.parametrize("rule,oracle_rule", RULES, ids=IDS)
def test_random_one_sided_pattern(rule, oracle_rule):
    A = one_sided(200, 7)
    S = A.scipy()
    assert (S != S.T).nnz > 0  # structurally non-symmetric
    colors = oracle_rule(A)
    assert not O.coloring_is_valid(A, colors)
    r, c = first_conflict(A, colors)
    mc = MCSOR(A.rowptr, A.colidx, A.vals, rule)
    with pytest.raises(PMGError) as e:
        mc.setup()
    assert e.value.code == 62
    assert f"rows {r} and {c} are coupled but share colour {colors[r]}" in str(e.value)
    mc.destroy()


@pytest.mark.parametrize("rule,oracle_rule", RULES, ids=IDS)
def test_oracle_twins_colour_the_symmetrised_pattern(rule, oracle_rule):
    """the oracle twin of every rule gives the symmetrised pattern a valid colouring.  The library is not called: its set-up
    would go on to the device.  test_gpu_aij_wide.py sets every rule up on symmetric matrices and compares the colourings
    with these twins."""
    A = one_sided(200, 7).scipy()
    A = O.CSR.from_scipy(A + A.T)
    assert O.coloring_is_valid(A, oracle_rule(A))
