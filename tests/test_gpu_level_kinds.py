"""What a set-up makes of every level, held to the level's KIND: which single-kernel entry points a level serves, its layout and
extents, the V-cycle byte model (total and per level, exact), whether the multi-chain cycle takes the hierarchy and what it charges,
and that a second setup() changes nothing.  Four smallest hierarchies that between them produce a grid, a class-stencil, a
sliced-ELL, a block-smoothed sliced-ELL and an exactly sampled level:

  dmda         9 x 9 x 9, three levels, default switches: grid / class stencil / exact
  dmda_gibbs   the same with a Gibbs coarsest level:       grid / class stencil / class stencil
  aij          9 x 9 five-point Laplacian, bilinear interpolation 9 -> 5 -> 3 per direction, Galerkin products: sliced-ELL /
               sliced-ELL / exact
  aij_blocks   the same with the grid lines as blocks on the finest level

EXPECTED was recorded from the library at commit 5d45c7b ("Test both block Gibbs kernels on colour launches of up to 65 tiles"),
the last one that inferred a level's kind from its flags at every use; `PYTHONPATH=. python tests/test_gpu_level_kinds.py`
prints it again."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
SEEDS = [11, 22, 33]
OPS = ("sweep", "residual", "restrict", "prolong_add", "residual_restrict")


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def _csr(m):
    m = sp.csr_matrix(m)
    m.sort_indices()
    return m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.astype(np.float64)


def _interp1d(nf):
    nc = (nf - 1) // 2 + 1
    P = sp.lil_matrix((nf, nc))
    for j in range(nc):
        P[2 * j, j] = 1.0
    for j in range(nc - 1):
        P[2 * j + 1, j] = P[2 * j + 1, j + 1] = 0.5
    return P.tocsr()


def laplace_hierarchy():
    """(operators, interpolations) of MGMC.from_hierarchy: 81, 25 and 9 rows"""
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(9, 9))
    A = [None, None, (sp.kron(sp.identity(9), T) + sp.kron(T, sp.identity(9)) + 0.5 * sp.identity(81)).tocsr()]
    P = [None, sp.kron(_interp1d(5), _interp1d(5)).tocsr(), sp.kron(_interp1d(9), _interp1d(9)).tocsr()]
    for l in (2, 1):
        A[l - 1] = (P[l].T @ A[l] @ P[l]).tocsr()
    return [_csr(a) for a in A], [None] + [_csr(p) for p in P[1:]]


def build(case):
    from parmgmc_amd import MGMC

    if case.startswith("dmda"):
        mg = MGMC(9, 9, 9, 1.0, 3)
    else:
        mg = MGMC.from_hierarchy(*laplace_hierarchy())
        if case == "aij_blocks":
            mg.set_level_blocks(2, [np.arange(9 * j, 9 * j + 9) for j in range(9)])
    if case == "dmda_gibbs":
        mg.set_coarse("gibbs", 2)
    return mg.setup()


CASES = ("dmda", "dmda_gibbs", "aij", "aij_blocks")


def status(call):
    from parmgmc_amd import PMGError

    try:
        call()
        return 0
    except PMGError as e:
        return e.code


def observe(mg):
    """everything the test holds to the recorded values, as plain lists and numbers"""
    import torch

    layouts = [list(mg.level_layout(l)) for l in range(mg.levels)]
    out = {"layout": layouts, "dims": [list(mg.level_dims(l)) for l in range(mg.levels)], "ops": []}
    for l in range(mg.levels):
        v = [torch.zeros(layouts[l][1], dtype=torch.float64, device="cuda") for _ in range(3)]
        c = torch.zeros(layouts[max(l - 1, 0)][1], dtype=torch.float64, device="cuda")  # level 0 has no coarser level: refused before any use
        calls = {
            "sweep": lambda: mg.level_sweep(l, v[0], v[1]),
            "residual": lambda: mg.level_residual(l, v[0], v[1], v[2]),
            "restrict": lambda: mg.level_restrict(l, v[0], c),
            "prolong_add": lambda: mg.level_prolong_add(l, c, v[0]),
            "residual_restrict": lambda: mg.level_residual_restrict(l, v[0], v[1], c),
        }
        out["ops"].append([status(calls[op]) for op in OPS])
    torch.cuda.synchronize()
    tot, per = mg.algorithmic_bytes()
    out["bytes"] = [tot, [float(x) for x in per]]
    Y = torch.zeros((mg.n, 3), dtype=torch.float64, device="cuda")
    out["chains"] = status(lambda: mg.sample_chains(dev(np.ones(mg.n)), Y, 1, SEEDS))
    out["bytes_chains"] = status(lambda: mg.algorithmic_bytes_chains(3))
    if out["bytes_chains"] == 0:
        tot, per = mg.algorithmic_bytes_chains(3)
        out["bytes_chains"] = [tot, [float(x) for x in per]]
    return out


# status codes of include/parmgmc_hip.h: 0 = PMG_SUCCESS, 56 = PMG_ERR_SUP, 63 = PMG_ERR_ARG_OUTOFRANGE (level 0 has no coarser level)
_NO_COARSER = [63, 63, 63]
EXPECTED = {
    "dmda": {
        "layout": [[3, 45, 9], [1, 175, 25], [0, 1188, 0]],
        "dims": [[3, 3, 3], [5, 5, 5], [9, 9, 9]],
        "ops": [[56, 56] + _NO_COARSER, [0, 0, 0, 0, 56], [56, 0, 0, 0, 0]],  # exact: nothing; class stencil: no fused step; grid: no sweep here
        "bytes": [71752.0, [5832.0, 11432.0, 54488.0]],
        "chains": 56,
        "bytes_chains": 56,
    },
    "dmda_gibbs": {
        "layout": [[1, 45, 9], [1, 175, 25], [0, 1188, 0]],
        "dims": [[3, 3, 3], [5, 5, 5], [9, 9, 9]],
        "ops": [[0, 0] + _NO_COARSER, [0, 0, 0, 0, 56], [56, 0, 0, 0, 0]],
        "bytes": [67432.0, [1512.0, 11432.0, 54488.0]],
        "chains": 56,
        "bytes_chains": 56,
    },
    "aij": {
        "layout": [[3, 9, 0], [2, 256, 0], [2, 128, 0]],
        "dims": [[9, 1, 1], [25, 1, 1], [81, 1, 1]],
        "ops": [[56, 56] + _NO_COARSER, [56, 0, 0, 0, 56], [56, 0, 0, 0, 56]],  # sliced-ELL: sweeps are pmg_mcsor's own entry points
        "bytes": [40544.0, [648.0, 11040.0, 28856.0]],
        "chains": 0,
        "bytes_chains": [61200.0, [1944.0, 16864.0, 42392.0]],
    },
    "aij_blocks": {
        "layout": [[3, 9, 0], [2, 256, 0], [2, 128, 0]],
        "dims": [[9, 1, 1], [25, 1, 1], [81, 1, 1]],
        "ops": [[56, 56] + _NO_COARSER, [56, 0, 0, 0, 56], [0, 0, 0, 0, 56]],  # the block sweep the cycle runs on the finest level
        "bytes": [131504.0, [648.0, 11040.0, 119816.0]],
        "chains": 56,
        "bytes_chains": 56,
    },
}


@pytest.mark.parametrize("case", CASES)
def test_level_kinds_as_recorded(case):
    got = observe(build(case))
    print(case, got)
    assert got == EXPECTED[case]


@pytest.mark.parametrize("case", CASES)
def test_second_setup_is_a_no_op(case):
    import torch

    mg = build(case)
    rng = np.random.default_rng(5)
    b, y0 = dev(rng.standard_normal(mg.n)), dev(rng.standard_normal(mg.n))
    before, y1 = observe(mg), y0.clone()
    assert mg.sample(b, y1, 2, seed=0xCAFE) == 2
    mg.setup()
    after, y2 = observe(mg), y0.clone()
    assert mg.sample(b, y2, 2, seed=0xCAFE) == 2
    assert before == after == EXPECTED[case]
    assert torch.equal(y1, y2) and bool(torch.isfinite(y1).all())


if __name__ == "__main__":
    import pprint

    pprint.pprint({case: observe(build(case)) for case in CASES}, width=160, compact=True)
