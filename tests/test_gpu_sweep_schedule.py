"""The sweep schedule as one API-level contract of all samplers: a symmetric call with its = 2 from draw counter 7 equals,
bit for bit, four single-direction calls with its = 1 at counters 7, 8, 9, 10 (forward, backward, forward, backward), and
returns counter 11.  Grid cvec, MCSOR on natural vectors, MCSOR on layout vectors and MCSOR on 3 chains, each without an
update and with a rank-2 low-rank (MATLRC) update, on a 9 x 9 x 5 grid (405 rows: odd plane count, partial wavefronts)."""
import ctypes as C

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
NX, NY, NZ, KAPPA = 9, 9, 5, 2.0
SEED, SEEDS, COUNTER0 = 0xC0FFEE, (11, 0xFFFFFFFF00000001, 12345), 7


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


class GridCvec:
    def __init__(self, B, S):
        from parmgmc_amd import GridMCSOR

        self.s = GridMCSOR(NX, NY, NZ, KAPPA)
        if B is not None:
            self.s.set_lowrank(B, S)

    def state(self, b, y):
        return self.s.to_cvec(dev(b)), self.s.to_cvec(dev(y))

    def sample(self, b, y, its, counter0):
        return self.s.sample_cvec(b, y, its, SEED, counter0)


class McsorNatural:
    def __init__(self, B, S):
        from parmgmc_amd import MCSOR

        A = O.shifted_laplace(NX, NY, NZ, KAPPA)
        self.s = MCSOR(A.rowptr, A.colidx, A.vals).setup()
        if B is not None:
            self.s.set_lowrank(B, S)

    def state(self, b, y):
        return dev(b), dev(y)

    def sample(self, b, y, its, counter0):
        return self.s.sample(b, y, its, SEED, counter0)


class McsorLayout(McsorNatural):
    def state(self, b, y):
        import torch

        from parmgmc_amd.capi import check, lib
        from parmgmc_amd.wrappers import _ptr, _stream

        out = []
        for v in (b, y):
            lay = torch.zeros(self.s.layout_len(), dtype=torch.float64, device="cuda")
            check(lib.pmg_mcsor_to_layout(self.s._h, _ptr(dev(v)), _ptr(lay), _stream()))
            out.append(lay)
        return tuple(out)

    def sample(self, b, y, its, counter0):
        from parmgmc_amd.capi import check, lib
        from parmgmc_amd.wrappers import _ptr, _stream

        out = C.c_uint64()
        check(lib.pmg_mcsor_sample_layout(self.s._h, _ptr(b), _ptr(y), its, 1, SEED, counter0, C.byref(out), _stream()))
        return out.value


class McsorChains(McsorNatural):
    def state(self, b, y):
        return dev(b), dev(np.stack([y, 2.0 * y, -y], axis=1))

    def sample(self, b, Y, its, counter0):
        return self.s.sample_chains(b, Y, its, SEEDS, counter0)


@pytest.fixture(scope="module")
def lowrank():
    from parmgmc_amd import make_observation_mats

    B, S, _ = make_observation_mats(NX, NY, NZ, [[0.3, 0.3, 0.4], [0.7, 0.6, 0.6]], [0.3, 0.25], [1.0, -0.5], 1e-2)
    assert B.shape == (NX * NY * NZ, 2) and (np.abs(B).sum(0) > 0).all()
    return B, S


@pytest.mark.parametrize("with_update", [False, True], ids=["plain", "lowrank2"])
@pytest.mark.parametrize("sampler", [GridCvec, McsorNatural, McsorLayout, McsorChains], ids=lambda s: s.__name__)
def test_symmetric_call_equals_four_directional_calls(sampler, with_update, lowrank):
    import torch

    from parmgmc_amd.capi import SOR_BACKWARD_SWEEP, SOR_FORWARD_SWEEP, SOR_SYMMETRIC_SWEEP

    rng = np.random.default_rng(5)
    b0, y0 = rng.standard_normal(NX * NY * NZ), rng.standard_normal(NX * NY * NZ)
    s = sampler(*(lowrank if with_update else (None, None)))
    b, y_sym = s.state(b0, y0)
    _, y_dir = s.state(b0, y0)
    assert torch.equal(y_sym, y_dir)

    s.s.set_sweep_type(SOR_SYMMETRIC_SWEEP)
    assert s.sample(b, y_sym, 2, COUNTER0) == COUNTER0 + 4
    assert not torch.equal(y_sym, y_dir)  # the chain moved

    for i, direction in enumerate((SOR_FORWARD_SWEEP, SOR_BACKWARD_SWEEP, SOR_FORWARD_SWEEP, SOR_BACKWARD_SWEEP)):
        s.s.set_sweep_type(direction)
        assert s.sample(b, y_dir, 1, COUNTER0 + i) == COUNTER0 + i + 1
    assert torch.equal(y_sym, y_dir)
    assert bool(torch.isfinite(y_sym).all())
