"""tests/rbstats_dmda_e2e.py without a GPU: the operator is the scaled ex6 operator it is said to be, and on the oracle's chain the
Rao-Blackwellised variance field is closer to diag(Q^-1) than the plain one by the margin the GPU test relies on."""
import numpy as np

import oracle as O
import rbstats_cases as R
import rbstats_dmda_e2e as E


def test_operator_is_the_scaled_ex6_operator():
    A = O.shifted_laplace(*E.E2E["grid"], E.E2E["kappa"]).scipy().toarray()
    X = O.ex6_matrix(33, 0.01).scipy().toarray() / 32**2
    assert np.abs(A - X).max() <= 4 * np.finfo(float).eps * np.abs(X).max()


def test_end_to_end_configuration_on_the_oracle_chain():
    """the configuration of the GPU end-to-end test on the oracle's restatement of the same chains: the variance ratio is at or
    below 0.9, so that the device chain's parity with the oracle cannot turn err_rb <= err_plain.
    Observed: variance err_plain 0.07625, err_rb 0.05733 (ratio 0.752); mean err_plain 0.04981, err_rb 0.04599 (ratio 0.923: the
    gain on the mean is small on this sampler, as DESIGN 11.5 found, and no assertion rests on it)."""
    C = E.E2E
    A, _, _, b = E.problem()
    chains = E.oracle_chains(C["burn_in"] + C["window"])
    X = chains[C["burn_in"] :].reshape(-1, A.n)
    assert X.shape == (C["window"] * C["nchains"], A.n)
    mp, mr, vp, vr = R.plain_and_rb_errors(A.scipy().toarray(), b, X)
    print(f"oracle chain: mean err_plain {mp:.5f} err_rb {mr:.5f} ratio {mr / mp:.3f}; variance err_plain {vp:.5f} err_rb {vr:.5f} ratio {vr / vp:.3f}")
    assert vr / vp <= 0.9
