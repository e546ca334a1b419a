"""The chain statistics kernels (kernels_chainstats.hip) at every lane split and launch geometry of tests/chainstats_cases.py:

  a. fields() and trace(q) bit for bit against the float64 emulation of the kernel header's ORDER OF EVERY SUM, at every chain
     count of CONTROLS + CHAINS (LPRL 0..6, the powers of two, the chunk edges 64 | 65 and 128 | 129) and at 64 | 65 blocks;
  b. several iterations per wavefront (the row index row0 + it * RWI + g, the QOI accumulated across iterations, the parked LDS
     slot of chunked chains at it > 0) per template, within the extended-precision bounds of check_against_longdouble;
  c. the iteration cap of chunked chains (more than 32 * 32 * 1024 rows, more than 1024 blocks) on integer samples generated on
     the device: the traces equal an int64 sum, the fields of sampled rows are within the bounds;
  d. negative controls: one changed entry moves its row's fields and its chain's QOI out of the bounds and nothing else by a bit;
  e. the same bits on a second run after reset() on a side stream.
Observed on the MI355X: a. every bit equal.  b. worst error / bound over the eleven cases: mean 0.112 (n = 2097153, C = 1),
variance 1.2e-3, QOI 2.3e-5 (n = 32769, C = 64).  c. traces equal; mean 4.2e-3, variance 9.5e-4 of the bound on 4060 rows."""
import numpy as np
import pytest

import chainstats_cases as K
from test_gpu_chainstats import check_against_longdouble, dev, make_qois, make_steps

pytestmark = pytest.mark.gpu
T = 3


def run(n, C, steps, qois):
    from parmgmc_amd import ChainStats

    cs = ChainStats(n, C, qois, max_steps=len(steps))
    for Y in steps:
        cs.update(dev(Y))
    assert cs.count() == (len(steps), len(steps) * C)
    return cs


# ---- a. bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0.0, 50.0])
@pytest.mark.parametrize("n,C", K.EXACT)
def test_bits_are_the_documented_order(n, C, offset):
    steps = make_steps(n, C, T, offset, seed=n + 7 * C + T)
    qois = make_qois(n, 4, seed=C)
    assert [w is None for w in qois] == [True, False, False, False]
    cs = run(n, C, steps, qois)
    em = K.emulate(steps, qois)
    mean, var = (t.cpu().numpy() for t in cs.fields())
    m_em, v_em = em.fields_host()
    label = f"n={n} C={C} offset={offset}"
    assert np.array_equal(mean, m_em), (label, "mean", int((mean != m_em).sum()), float(np.abs(mean - m_em).max()))
    assert np.array_equal(var, v_em), (label, "var", int((var != v_em).sum()), float(np.abs(var - v_em).max()))
    for q in range(4):
        got, want = cs.trace(q), em.trace(q)
        assert np.array_equal(got, want), (label, "qoi", q, int((got != want).sum()), float(np.abs(got - want).max()))
    check_against_longdouble(cs, steps, qois, label)


# ---- b. several iterations per wavefront ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C,why", K.MULTI_ITER, ids=[f"{n}-{C}" for n, C, _ in K.MULTI_ITER])
def test_several_iterations_per_wavefront(n, C, why):
    lprl, chunks, iters, nb, rpw = K.geometry(n, C)
    want = {(70001, 128): (2, 3), (40000, 129): (3, 2), (32769, 65): (2, 2)}.get((n, C), (1, 2))
    assert (chunks, iters) == want and nb <= K.MAXBLK, (why, chunks, iters, nb)
    steps = make_steps(n, C, T, 50.0, seed=n + C)
    qois = make_qois(n, 2, seed=C)
    check_against_longdouble(run(n, C, steps, qois), steps, qois, f"n={n} C={C} LPRL={lprl} chunks={chunks} iters={iters}")


# ---- c. the cap ------------------------------------------------------------------------------------------------------------------------
class _Rows:
    """fields() of a handle at some rows only"""

    def __init__(self, cs, rows):
        self.cs, self.rows = cs, rows

    def fields(self):
        return tuple(f[self.rows] for f in self.cs.fields())


def test_iteration_cap_of_chunked_chains():
    import torch

    from parmgmc_amd import ChainStats

    n, C = K.CAP_CASE
    lprl, chunks, iters, nb, rpw = K.geometry(n, C)
    assert (lprl, chunks, iters, nb, rpw) == (6, 2, K.ITER_CAP, 1057, K.MAXRPW) and K.uncapped_iters(n, C) > K.ITER_CAP and nb > K.MAXBLK
    steps_n = 2
    rng = np.random.default_rng(5)
    regions = -(-n // rpw)
    picked = []
    for reg in (0, regions // 2, regions - 2):  # whole wavefront regions: first and last row, it = 0, 1, 31
        base = reg * rpw
        picked += [base, base + rpw - 1] + [base + it * K.RW + i for it in (0, 1, K.ITER_CAP - 1) for i in range(K.RW)]
    picked += [(regions - 1) * rpw, n - 1] + list(range(n - 64, n)) + list(rng.integers(0, n, 4096 - 160))
    rows_h = np.unique(np.clip(picked, 0, n - 1))
    assert 3500 <= len(rows_h) <= 4096 and (regions - 1) * rpw == n - 1  # the last wavefront has one row
    rows = torch.as_tensor(rows_h, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(11)
    w_h = rng.integers(-4, 5, n).astype(np.float64)
    w_i = torch.as_tensor(w_h, device="cuda").to(torch.int64)
    cs = ChainStats(n, C, [None, w_h], max_steps=steps_n)
    sampled, sums = [], []
    for _ in range(steps_n):
        Y = torch.randint(-8, 9, (n, C), device="cuda", dtype=torch.float64, generator=gen)
        Y += torch.randint(-50, 51, (n, 1), device="cuda", dtype=torch.float64, generator=gen)  # every row its own level
        cs.update(Y)
        sampled.append(Y[rows].cpu().numpy())
        s0, s1 = torch.zeros(C, dtype=torch.int64, device="cuda"), torch.zeros(C, dtype=torch.int64, device="cuda")
        for r0 in range(0, n, 1 << 17):  # int64 sums in row slabs: no second array of this size
            Yi = Y[r0 : r0 + (1 << 17)].to(torch.int64)
            s0 += Yi.sum(0)
            s1 += (w_i[r0 : r0 + (1 << 17), None] * Yi).sum(0)
        sums.append((s0.cpu().numpy(), s1.cpu().numpy()))
        del Y, Yi
    for q in range(2):
        tr = cs.trace(q)
        assert tr.shape == (steps_n, C)
        for t in range(steps_n):
            assert np.abs(sums[t][q]).max() < 2**53 and np.abs(sums[t][q]).max() > 0
            assert np.array_equal(tr[t], sums[t][q].astype(np.float64)), (q, t, np.abs(tr[t] - sums[t][q]).max())
    check_against_longdouble(_Rows(cs, rows), sampled, [], f"cap n={n} C={C} iters={iters} blocks={nb}, {len(rows_h)} rows")
    torch.cuda.synchronize()


# ---- d. negative controls --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C", K.NEGATIVE)
def test_one_changed_entry_is_seen_where_it_belongs(n, C):
    """the last entry of the last step, and an entry at it = 1 (where the case has a second iteration) of chunk 1 (where it has
    one): changed by 8 away from the row's mean"""
    lprl, chunks, iters, nb, rpw = K.geometry(n, C)
    G = 64 >> lprl
    steps = make_steps(n, C, T, 50.0, seed=n + C)
    qois = make_qois(n, 2, seed=C)
    cs = run(n, C, steps, qois)
    mean0, var0 = (t.cpu().numpy() for t in cs.fields())
    tr0 = [cs.trace(q) for q in range(2)]
    m_ref, v_ref, mean_bound, var_bound = K.longdouble_fields(steps)
    it = min(1, iters - 1)
    inner = (5 * rpw + it * G * K.RW + 3, 64 if chunks > 1 else 5)
    assert inner[0] < n - 1 and inner[0] % rpw // (G * K.RW) == it and inner[1] // 64 == min(1, chunks - 1)
    if (n, C) == (32769, 65):
        assert it == 1 and inner[1] // 64 == 1
    for r, c in ((n - 1, C - 1), inner):
        changed = [Y.copy() for Y in steps]
        changed[-1][r, c] += 8.0 if changed[-1][r, c] >= float(m_ref[r]) else -8.0
        m_new, v_new, _, _ = K.longdouble_fields([Y[r : r + 1] for Y in changed])
        assert abs(m_new[0] - m_ref[r]) >= 100 * mean_bound and abs(v_new[0] - v_ref[r]) >= 100 * var_bound  # the reference moves
        cs1 = run(n, C, changed, qois)
        mean1, var1 = (t.cpu().numpy() for t in cs1.fields())
        others = np.arange(n) != r
        assert np.array_equal(mean1[others], mean0[others]) and np.array_equal(var1[others], var0[others]), (r, c)
        e_m, e_v = float(abs(mean1[r] - m_ref[r])), float(abs(var1[r] - v_ref[r]))
        print(f"n={n} C={C} entry ({r}, {c}): mean off by {e_m / mean_bound:.3e} bounds, var by {e_v / var_bound:.3e} bounds")
        assert e_m > mean_bound and e_v > var_bound, (r, c, e_m, e_v)
        moved = []
        for q, w in enumerate(qois):
            tr1 = cs1.trace(q)
            same = np.ones((T, C), bool)
            same[-1, c] = False
            assert np.array_equal(tr1[same], tr0[q][same]), (r, c, q)
            ref, bound = K.longdouble_qoi(steps[-1], w, c)
            ref_new, _ = K.longdouble_qoi(changed[-1], w, c)
            if abs(ref_new - ref) >= 100 * bound:
                moved.append(q)
                assert abs(tr1[-1, c] - ref) > bound, (r, c, q)
                print(f"n={n} C={C} entry ({r}, {c}): qoi {q} off by {float(abs(tr1[-1, c] - ref) / bound):.3e} bounds")
        assert 0 in moved, (r, c, moved)  # the all-ones QOI moves by 8


# ---- e. determinism --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C", K.TWICE)
def test_same_bits_twice(n, C):
    import torch

    from parmgmc_amd import ChainStats

    steps = [dev(Y) for Y in make_steps(n, C, T, 50.0, seed=C)]
    qois = make_qois(n, 2, seed=1)
    cs = ChainStats(n, C, qois, max_steps=T)
    for Y in steps:
        cs.update(Y)
    m1, v1 = cs.fields()
    t1 = [cs.trace(q) for q in range(2)]
    torch.cuda.synchronize()
    cs.reset()
    assert cs.count() == (0, 0)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for Y in steps:
            cs.update(Y)
        m2, v2 = cs.fields()
    st.synchronize()
    assert torch.equal(m1, m2) and torch.equal(v1, v2)
    for q in range(2):
        assert np.array_equal(t1[q], cs.trace(q))
