"""Workloads of tests/test_gpu_mgmc_lowrank_chains.py and tests/test_gpu_chain_lane_splits.py: MGMC hierarchies with a low-rank (MATLRC) update for the many-chains
V-cycle.  The observation recipes are those of tests/test_gpu_lowrank_chains.py (copied: that module is a test file), the
delay / stream-pair helpers those of tests/test_gpu_stream_contract.py; the byte formula restates the comment of
pmg_mgmc_get_algorithmic_bytes_chains."""
import contextlib
import gc
from pathlib import Path

import numpy as np
import pytest

import oracle as O

GOLD = Path(__file__).resolve().parent / "golden"
SEEDS = [0xBEEF + 1009 * c for c in range(80)]
LSHAPE_BALLS = [(0.5, 0.5), (1.5, 0.5), (0.5, 1.5)]  # inside the L: [0, 2]^2 without [1, 2]^2
GRID17 = (17, 17, 9)
ROWS_PER_BLOCK = 1024  # support rows one block of the compact B^T y kernels sums (pmgk_lrc_rows_per_block)
DENSE_ROWS_PER_BLOCK = 4096
DELAY_N, DELAY_REPS = 4096, 24


def dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, np.float64), device="cuda")


def grid_balls(grid, centres, radius):
    """ball indicators on the unit-cube grid, natural order with x fastest"""
    nx, ny, nz = grid
    X, Y, Z = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny), np.linspace(0, 1, nz), indexing="ij")
    pts = np.stack([X.ravel(order="F"), Y.ravel(order="F"), Z.ravel(order="F")], 1)
    return [((pts - np.asarray(c)) ** 2).sum(1) < radius * radius for c in centres]


def observations_17(form, k, seed):
    """B (n x k) and S on the 17 x 17 x 9 grid.  rows: the k columns are random weights on two small balls (the row-compact form);
    wide: every column on a third of the rows (the dense form)."""
    n = int(np.prod(GRID17))
    rng = np.random.default_rng(seed)
    B = np.zeros((n, k))
    if form == "wide":
        for j in range(k):
            idx = rng.choice(n, size=n // 3, replace=False)
            B[idx, j] = rng.uniform(0.5, 1.5, len(idx)) / len(idx)
    else:
        balls = grid_balls(GRID17, [(0.3, 0.3, 0.4), (0.7, 0.6, 0.6)], 0.16)
        for j in range(k):
            inside = balls[j % 2]
            B[inside, j] = rng.uniform(0.5, 1.5, inside.sum()) / inside.sum()
    return B, rng.uniform(20.0, 90.0, k)


_HIER17 = []


def hierarchy_17():
    """the 17 x 17 x 9 shifted Laplacian and its aggregation hierarchy with coarse_max = 100 (built once)"""
    from parmgmc_amd.unstructured import build_hierarchy

    if not _HIER17:
        A = O.shifted_laplace(*GRID17, 2.0)
        ops, ps = build_hierarchy(A.scipy().tocsr(), coarse_max=100)
        assert len(ops) >= 3, [len(o[0]) - 1 for o in ops]
        _HIER17.append((A, ops, ps))
    return _HIER17[0]


def make_mgmc(ops, ps, lowrank=None, coarse="cholsampler", omega=1.0, scaled=True, sweep=1, nu=1, coarse_its=1, coloring=None):
    """set-up MGMC on a caller-supplied hierarchy, with the update (B, S) on every level when given"""
    from parmgmc_amd import MGMC

    mg = MGMC.from_hierarchy(ops, ps)
    if coloring is not None:
        mg.set_coloring(coloring)
    mg.set_smoother(scaled, omega, sweep, nu)
    mg.set_coarse(coarse, coarse_its)
    if lowrank is not None:
        mg.set_lowrank(*lowrank)
    return mg.setup()


def level_lowrank_sizes(mg, ops, level):
    """(k, rows the level's low-rank passes run over, dense): MGMC.level_lowrank_sizes (level_lowrank_factors serves grid and
    class-stencil levels only); the dense form runs over all rows of the level"""
    k, rows, dense = mg.level_lowrank_sizes(level)
    assert not dense or rows == len(ops[level][0]) - 1
    return k, rows, dense


def lowrank_chain_bytes(mg, ops, k, C, coarse, nu, ndir, coarse_its, literal):
    """what the update adds to the algorithmic bytes of one chains V-cycle (comment of pmg_mgmc_get_algorithmic_bytes_chains)"""
    top, total = len(ops) - 1, 0.0
    for l in range(len(ops)):
        if l == 0 and coarse == "cholsampler":
            continue  # the exact sampler factors the explicit sum
        _, n, dense = level_lowrank_sizes(mg, ops, l)
        N = len(ops[l][0]) - 1
        idx = 0.0 if dense else 8.0 * n
        nb = -(-N // DENSE_ROWS_PER_BLOCK) if dense else -(-n // ROWS_PER_BLOCK)
        s = 2 * nu * ndir if l >= 1 else coarse_its * ndir
        noise = 8.0 * k * n + idx + 8.0 * k * C + 24.0 * n * C
        upd = 8.0 * k * n + idx + 8.0 * k * C + 16.0 * n * C
        btx = 8.0 * k * n + idx + 8.0 * n * C + 8.0 * nb * k * C
        red = 8.0 * nb * k * C + 8.0 * k * C
        one = 16.0 * k * n + idx + 24.0 * n * C
        fused = not dense and n <= ROWS_PER_BLOCK
        repair = one + 16.0 * n * C if fused else btx + red + upd + 16.0 * n * C
        resid = one + 8.0 * k if fused else btx + red + 8.0 * k + upd
        total += s * (noise + repair) + 8.0 * k * C * s + 8.0 * C
        if l >= 1:
            total += resid
        if l == top:
            total += 8.0 * k + (resid if literal else 2 * nu * ndir * (8.0 * N * C - 8.0 * N))
    return total


@pytest.fixture(scope="module")
def config4():
    """BASELINE config 4 (bench.py's unstructured_secondary): lshape.msh refined 5 times, P1 kappa^2 M + K, the aggregation
    hierarchy with coarse_max = 2000; plus three ball observations of ~3700 vertices each"""
    from parmgmc_amd.unstructured import assemble_p1, ball_observations, build_hierarchy, read_gmsh41_triangles, refine_uniform

    xy, tris = read_gmsh41_triangles(GOLD / "lshape.msh")
    for _ in range(5):
        xy, tris = refine_uniform(xy, tris)
    A = assemble_p1(xy, tris, 1.0)
    ops, ps = build_hierarchy(A, coarse_max=2000)
    B = ball_observations(xy, LSHAPE_BALLS, 0.1)
    assert ((B > 0).sum(0) > 3000).all()
    return A, ops, ps, B, np.array([40.0, 60.0, 80.0]), {}


def ex6_posterior():
    """the operator, observations and seeds of test_ex6_shape_posterior_covariance (tests/test_gpu_lowrank_chains.py)"""
    A = O.ex6_matrix(32, 1e-2)
    n, nchains = A.n, 1000
    side = int(round(np.sqrt(n)))
    X, Yg = np.meshgrid(np.linspace(0, 1, side), np.linspace(0, 1, side), indexing="ij")
    pts = np.stack([X.ravel(order="F"), Yg.ravel(order="F")], 1)
    B = np.zeros((n, 3))
    for j, ctr in enumerate([(0.25, 0.3), (0.7, 0.5), (0.4, 0.8)]):
        inside = ((pts - np.asarray(ctr)) ** 2).sum(1) < 0.2**2
        B[inside, j] = 1.0 / inside.sum()
    S = np.array([1e4, 2e4, 5e4])
    Ad = A.scipy().toarray()
    post = np.linalg.inv(Ad + B @ np.diag(S) @ B.T)
    prior = np.linalg.inv(Ad)
    seeds = [0x5EED0000 + 7919 * c for c in range(nchains)]
    fro = np.linalg.norm(post)
    mc_err = np.sqrt((fro**2 + np.trace(post) ** 2) / (nchains - 1)) / fro
    return A, B, S, post, prior, seeds, mc_err


def cov_err(Ys, Sigma, post):
    """||C_N - Sigma||_F / ||(A + B S B^T)^-1||_F for the sample covariance C_N over the chains"""
    X = Ys.T.contiguous().cpu().numpy()
    return np.linalg.norm(np.cov(X, rowvar=False) - Sigma) / np.linalg.norm(post)


# ---- the slow-producer pattern of tests/test_gpu_stream_contract.py -----------------------------------------------------------
@pytest.fixture(scope="module")
def delay():
    """enqueue() queues about 50 ms of ordinary torch work on the current stream"""
    import torch

    a = torch.randn((DELAY_N, DELAY_N), dtype=torch.float64, device="cuda") / DELAY_N**0.5
    scratch = torch.empty_like(a)

    def enqueue():
        for _ in range(DELAY_REPS):
            torch.mm(a, a, out=scratch)

    enqueue()  # loads the BLAS kernels
    torch.cuda.synchronize()
    return enqueue


@contextlib.contextmanager
def no_collection():
    """no cyclic garbage collection inside: one that frees a handle calls hipFree, which waits for the whole device"""
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        gc.enable()


@pytest.fixture(scope="module")
def streams(delay):
    """(side, third): two streams that run concurrently"""
    import torch

    side = torch.cuda.Stream()
    poison = torch.full((4096,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(16):
        third = torch.cuda.Stream()
        behind, beside = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(side):
            delay()
            behind.record()
        with torch.cuda.stream(third):
            seen = poison.clone()
            beside.record()
        beside.synchronize()
        concurrent = not behind.query()
        torch.cuda.synchronize()
        del seen
        if concurrent:
            return side, third
    pytest.fail("no two streams of this process run concurrently")


# ---- a small hierarchy with BOTH compact chain kernels (tests/test_gpu_chain_lane_splits.py) ------------------------------------
LSHAPE3_BALLS = {3: (LSHAPE_BALLS, 0.2), 5: (LSHAPE_BALLS + [(1.0, 0.5), (0.5, 1.0)], 0.15)}  # k: (centres inside the L, radius)
_LSHAPE3 = []


def lshape3(k):
    """lshape.msh refined 3 times (23 809 vertices), P1 kappa^2 M + K, the aggregation hierarchy with coarse_max = 500 (four
    levels), and k ball observations whose joint support is several 1024-row blocks on the fine level, below a quarter of its
    rows (the row-compact form), and one block or less further down: (A, ops, ps, B, S)"""
    from parmgmc_amd.unstructured import assemble_p1, ball_observations, build_hierarchy, read_gmsh41_triangles, refine_uniform

    if not _LSHAPE3:
        xy, tris = read_gmsh41_triangles(GOLD / "lshape.msh")
        for _ in range(3):
            xy, tris = refine_uniform(xy, tris)
        A = assemble_p1(xy, tris, 1.0)
        _LSHAPE3.append((xy, A) + tuple(build_hierarchy(A, coarse_max=500)))
    xy, A, ops, ps = _LSHAPE3[0]
    centres, radius = LSHAPE3_BALLS[k]
    B = ball_observations(xy, centres, radius)
    support = int((B != 0).any(1).sum())
    assert 2 * ROWS_PER_BLOCK < support < A.shape[0] // 5, support
    return A, ops, ps, B, np.linspace(40.0, 80.0, k)
