"""End to end on a DMDA handle: the comparison of tests/test_gpu_rbstats.py::test_end_to_end_rb_beats_plain_moments with the
Rao-Blackwellised fields taken from pmg_rbstats_create_dmda.  The configuration (tests/rbstats_dmda_e2e.py) was fixed on the CPU
from the oracle's chain, where err_rb / err_plain of the variance field is 0.752 (tests/test_rbstats_dmda_e2e.py asserts <= 0.9)."""
import numpy as np
import pytest

import rbstats_cases as R
import rbstats_dmda_e2e as E

pytestmark = pytest.mark.gpu


def test_end_to_end_rb_variance_beats_plain_moments():
    """8 chains of MGMC on the 33 x 33 x 1 DMDA operator, stats= and rb= (a DMDA handle) together after the burn-in: the
    Rao-Blackwellised variance field is no further from diag(Q^-1) than the plain one -- the condition of the CSR handle's
    end-to-end test, not a tolerance -- and a CSR handle fed by the same run holds the same bits.
    Observed on the MI355X: variance err_plain 0.07625, err_rb 0.05733; mean err_plain 0.04981, err_rb 0.04599 (the figures of the
    oracle's chain on the CPU to all digits shown)."""
    import torch

    from parmgmc_amd import MGMC, ChainStats, RBStats

    C = E.E2E
    A, ops, ps, b = E.problem()
    mg = MGMC.from_hierarchy(ops, ps)
    mg.set_smoother(True, 1.0, 1, 1)
    mg.setup()
    n, nchains = A.n, C["nchains"]
    bd = torch.as_tensor(b, device="cuda")
    Sigma = np.linalg.inv(A.scipy().toarray())
    mu = Sigma @ b

    def run(rb):
        cs = ChainStats(n, nchains, [], max_steps=max(C["burn_in"], C["window"]))
        Y = torch.zeros((n, nchains), dtype=torch.float64, device="cuda")
        ctr = mg.sample_chains(bd, Y, C["burn_in"], C["seeds"], stats=cs, rb=rb)
        cs.reset()
        rb.reset()
        mg.sample_chains(bd, Y, C["window"], C["seeds"], counter0=ctr, stats=cs, rb=rb)
        assert cs.count() == rb.count() == (C["window"], C["window"] * nchains)
        return cs.fields(), rb.fields()

    (pm, pv), (rm, rv) = run(RBStats.dmda(*C["grid"], C["kappa"], nchains, b=bd))
    _, (cm, cv) = run(RBStats(A, nchains, b=bd))
    assert torch.equal(rm, cm) and torch.equal(rv, cv)
    pm, pv, rm, rv = (t.cpu().numpy() for t in (pm, pv, rm, rv))
    vp, vr = R.rel2(pv, np.diag(Sigma)), R.rel2(rv, np.diag(Sigma))
    mp, mr = R.rel2(pm, mu), R.rel2(rm, mu)
    print(f"end to end: variance err_plain {vp:.5f} err_rb {vr:.5f}; mean err_plain {mp:.5f} err_rb {mr:.5f}")
    assert np.isfinite(rv).all() and vr <= vp, (vr, vp)
