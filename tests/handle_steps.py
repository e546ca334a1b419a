"""A catalogue of steps per handle kind, for tests/test_gpu_call_history.py: the header's contract that a call's results depend on
the object's construction, its current settings and the call's arguments only -- not on what was called before.

  step     Step(name, fn, const, calls): fn(handle, x) -> {tag: tensor | int | float | numpy array | "not supported"} makes
           fresh output tensors from the read-only inputs x and leaves the handle's SETTINGS as it found them (a setter step is
           "set, call, set back"); const names the entries of x the call declares const; calls names the methods of
           parmgmc_amd/wrappers.py (Class.method) and of parmgmc_amd/pc.py the step goes through
  subject  one handle kind at one case: build() -> handle, inputs() -> x (device tensors; other entries are settings), the steps,
           and the calls the host refuses before any launch with the status the header documents (failing)

set_lowrank "uses the CURRENT omega" (pmg_grid.c, as the reference's MCSORSetUp), so the order omega -> set_lowrank is part of a
configuration: a step that changes omega on an object with a low-rank update re-issues set_lowrank when it sets omega and again
when it sets it back.  On the low-rank handles a second right-hand side, b_special, carries -0.0, a denormal and 1e300 on support
rows of the update: putting the right-hand side back must be a copy, not an arithmetic undo.  1e300 swamps the O(1) noise in every
entry a V-cycle touches (and may overflow), so only the "_special" steps run on it; every other step runs on an ordinary b, stays
finite and carries the noise.  The library keeps an update in the row-compact form -- the one that writes the noise term into the
caller's b in place -- when the joint support of B and of the sweeps applied to B is at most a quarter of the rows.
observations(..., "rows") on the grids and on lap6x5x4 is above that, so the "_lines3" / "_compact3" cases and the AIJ "_k3" cases
put B on a few neighbouring rows (clustered); ROW_COMPACT lists the cases that must be row-compact, and test_alone asserts the form
of every low-rank case with the lowrank_sizes queries.  The PC results are compared PC against PC (a PC alone against the same PC
type in any order, on the same noise stream); tests/test_gpu_pc_options.py ties the PCs to the samplers underneath.

Two results are legitimately history dependent and get their own bracket: the PC's noise counter (every PC step starts with
pmg_pc_set_noise_counter, and with the global seed that gives the PC the stream PC_SEED whatever its creation index) and the
accumulators' running sums (every ChainStats / ChainCov step starts with reset).

The builders and inputs are those of tests/test_gpu_stream_contract.py.  Left out: the distributed objects (pmg_dist*,
pmg_distmcsor*, row blocks), which need several processes.  This module holds no test functions and imports without a GPU."""
import contextlib
from collections import namedtuple

import numpy as np

import pair_front_workloads as PF
import test_gpu_stream_contract as SC

Step = namedtuple("Step", "name fn const calls")
Failing = namedtuple("Failing", "name fn status")  # fn(handle, x) -> status of a call the host refuses before any launch
Subject = namedtuple("Subject", "kind case build inputs steps failing")
ARG_OUTOFRANGE, ARG_NULL, SUP, ARG_WRONGSTATE = 63, 85, 56, 73  # PMG_ERR_* of include/parmgmc_hip.h
SEEDS = SC.SEEDS
SPECIAL = (-0.0, 5e-324, 1e300)  # on support rows of b_special on the low-rank handles
PC_SEED = 0x5EED0F0DD5
PERMUTATION_SEEDS = (101, 202, 303)


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def status(call):
    """the status of a wrapper call (0, or the code of the PMGError it raises)"""
    from parmgmc_amd import PMGError

    try:
        call()
        return 0
    except PMGError as e:
        return e.code


def or_not_supported(call, code=SUP):
    """run call(); the recorded result of an operation the object does not have (decided on the host) is "not supported" """
    from parmgmc_amd import PMGError

    try:
        return call()
    except PMGError as e:
        assert e.code == code, e
        return "not supported"


def zeros(n):
    import torch

    return torch.zeros(n, dtype=torch.float64, device="cuda")


def special_rows(b, B):
    """b with SPECIAL on the first support rows of the update B"""
    rows = np.flatnonzero(np.abs(B).sum(axis=1) > 0)
    b = b.copy()
    b[rows[: len(SPECIAL)]] = SPECIAL
    return b


def has_special(b):
    """the bit patterns of SPECIAL are in the host array b"""
    bits = np.ascontiguousarray(b, np.float64).view(np.int64)
    return all((bits == np.float64(v).view(np.int64)).any() for v in SPECIAL)


def clustered(n, row_sets, seed):
    """B (n x k), S with column j on the few rows row_sets[j]: a support (with that of the sweeps applied to B) of less than a
    quarter of the rows, which the library keeps in the row-compact form -- the form that writes the noise term into b in place"""
    rng = np.random.default_rng(seed)
    B = np.zeros((n, len(row_sets)))
    for j, rows in enumerate(row_sets):
        B[rows, j] = rng.uniform(0.5, 1.5, len(rows)) / len(rows)
    return B, rng.uniform(20.0, 90.0, len(row_sets))


@contextlib.contextmanager
def watch_seeds(seen):
    """every host seed array the wrappers hand to a chains entry point inside, appended to seen as (array, copy)"""
    from parmgmc_amd import wrappers

    orig = wrappers._seeds

    def recording(seeds, nchains):
        s = orig(seeds, nchains)
        seen.append((s, s.copy()))
        return s

    wrappers._seeds = recording
    try:
        yield seen
    finally:
        wrappers._seeds = orig


def orders(names):
    """{id: order}: the listed order, its reverse, and one permutation per seed of PERMUTATION_SEEDS"""
    out = {"listed": list(names), "reversed": list(names)[::-1]}
    for seed in PERMUTATION_SEEDS:
        out[f"perm{seed}"] = [names[i] for i in np.random.default_rng(seed).permutation(len(names))]
    return out


def _special(call, **keys):
    """a step: call(h, x) with the inputs keys[k] in the place of k (the right-hand side that carries SPECIAL), tags + "_special".
    1e300 swamps the noise and may overflow: these steps are for the restore of b; the steps on the ordinary b carry the noise"""

    def fn(h, x):
        xs = {**x, **{k: x[v] for k, v in keys.items()}}
        return {tag + "_special": v for tag, v in call(h, xs).items()}

    return fn


def _omega_bracket(h, x, omega, sweep_type):
    """set omega and the sweep type; an object with a low-rank update takes set_lowrank again (it uses the current omega)"""
    h.set_omega(omega)
    if x.get("lowrank") is not None:
        h.set_lowrank(*x["lowrank"])
    h.set_sweep_type(sweep_type)


def _symmetric_omega(call):
    """a step: call(h, x) with symmetric sweeps at omega 1.3, then forward sweeps at omega 1 again"""

    def fn(h, x):
        _omega_bracket(h, x, 1.3, 3)
        try:
            return call(h, x)
        finally:
            _omega_bracket(h, x, 1.0, 1)

    return fn


# ---- GridMCSOR ----------------------------------------------------------------------------------------------------------------
# (nx, ny, nz, kappa, update): "rows" = observations(..., "rows"), "lines" = three short x-lines (row-compact)
PAIR = PF.RANGE_SHAPES[0] + (PF.KAPPA,)  # 256 x 9 x 5: the plane-pair noisy kernel
assert PAIR[:3] == (256, 9, 5) and PAIR[:3] in PF.SHAPES
GRID_CASES = {**{k: v + (None,) for k, v in SC.GRIDS.items()}, "pair256x9x5": PAIR + (None,), "33x7x3_k3": SC.GRIDS["33x7x3"] + ("rows",), "pair256x9x5_k3": PAIR + ("rows",),
              "33x7x3_lines3": SC.GRIDS["33x7x3"] + ("lines",), "pair256x9x5_lines3": PAIR + ("lines",)}


def _grid_lowrank(case):
    nx, ny, nz, _, lowrank = GRID_CASES[case]
    if lowrank == "lines":  # natural order, x fastest: 5 neighbours in x on three (y, z) lines
        return clustered(nx * ny * nz, [np.arange(i0, i0 + 5) + nx * (j + ny * k) for i0, j, k in ((3, 1, 0), (nx // 2, ny - 2, nz - 1), (nx - 9, ny // 2, 1))], 35)
    return SC.observations(nx * ny * nz, 3, "rows", 31) if lowrank else None


def build_grid(case):
    from parmgmc_amd import GridMCSOR

    nx, ny, nz, kappa, lowrank = GRID_CASES[case]
    g = GridMCSOR(nx, ny, nz, kappa)
    if lowrank:
        g.set_lowrank(*_grid_lowrank(case))
    return g


def grid_inputs(case):
    from parmgmc_amd import GridMCSOR

    nx, ny, nz, kappa, lowrank = GRID_CASES[case]
    rng = np.random.default_rng(2)
    b, y = rng.standard_normal(nx * ny * nz), rng.standard_normal(nx * ny * nz)
    lr = _grid_lowrank(case)
    x = SC.to_dev({"b": b, "y": y})
    g = GridMCSOR(nx, ny, nz, kappa)  # the cvec layout depends on the dimensions alone
    x["bc"], x["yc"] = g.to_cvec(x["b"]), g.to_cvec(x["y"])
    if lowrank:
        x["b_special"] = SC.dev(special_rows(b, lr[0]))
        x["bc_special"] = g.to_cvec(x["b_special"])
    x["lowrank"] = lr
    return x


def _grid_apply(g, x):
    y = x["y"].clone()
    g.apply(x["b"], y)
    return {"apply": y}


def _grid_sample(g, x):
    y = x["y"].clone()
    return {"sample_ctr": g.sample(x["b"], y, 2, seed=0xCAFE, counter0=1), "sample": y}


def _grid_to_cvec(g, x):
    out = zeros(g.cvec_len)
    g.to_cvec(x["b"], out)
    return {"to_cvec": out, "from_cvec": g.from_cvec(x["bc"])}


def _grid_residual_cvec(g, x):
    r = zeros(g.cvec_len)
    g.residual_cvec(x["bc"], x["yc"], r)
    return {"residual_cvec": r, "residual": g.from_cvec(r)}


def _grid_apply_cvec(g, x):
    y = x["yc"].clone()
    g.apply_cvec(x["bc"], y)
    return {"apply_cvec": y, "apply_cvec_natural": g.from_cvec(y)}


def _grid_sample_cvec(g, x):
    y = x["yc"].clone()
    return {"sample_cvec_ctr": g.sample_cvec(x["bc"], y, 2, seed=0xCAFE, counter0=7), "sample_cvec": y}


def _grid_colour_sweeps(g, x):
    y = x["yc"].clone()
    for colour in (0, 1):
        g.sweep_color_cvec(colour, x["bc"], y, noisy=True, seed=3, counter=2)
    return {"colour_sweeps": y}


def _grid_plane_sweeps(g, x):
    y = x["yc"].clone()
    g.sweep_color_planes_cvec(0, 1, g.nz - 1, x["bc"], y, noisy=True, seed=3, counter=5)
    g.sweep_color_planes_cvec(1, 0, 1, x["bc"], y)
    return {"plane_sweeps": y}


def grid_steps(case):
    steps = [Step("apply", _grid_apply, ["b", "y"], ["GridMCSOR.apply"]), Step("sample", _grid_sample, ["b", "y"], ["GridMCSOR.sample"]),
             Step("sample_symmetric_omega1.3", _symmetric_omega(_grid_sample), ["b", "y"], ["GridMCSOR.sample"]), Step("to_cvec", _grid_to_cvec, ["b", "bc"], ["GridMCSOR.to_cvec", "GridMCSOR.from_cvec"]),
             Step("residual_cvec", _grid_residual_cvec, ["bc", "yc"], ["GridMCSOR.residual_cvec"]), Step("apply_cvec", _grid_apply_cvec, ["bc", "yc"], ["GridMCSOR.apply_cvec"]),
             Step("sample_cvec", _grid_sample_cvec, ["bc", "yc"], ["GridMCSOR.sample_cvec"]), Step("sample_cvec_symmetric_omega1.3", _symmetric_omega(_grid_sample_cvec), ["bc", "yc"], ["GridMCSOR.sample_cvec"])]
    if GRID_CASES[case][4] is not None:
        steps += [Step("sample_special", _special(_grid_sample, b="b_special"), ["b_special", "y"], ["GridMCSOR.sample"]),
                  Step("sample_cvec_special", _special(_grid_sample_cvec, bc="bc_special"), ["bc_special", "yc"], ["GridMCSOR.sample_cvec"])]
    if GRID_CASES[case][4] is None:  # the per-colour sweeps do not carry the low-rank repair
        steps += [Step("colour_sweeps", _grid_colour_sweeps, ["bc", "yc"], ["GridMCSOR.sweep_color_cvec"]), Step("plane_sweeps", _grid_plane_sweeps, ["bc", "yc"], ["GridMCSOR.sweep_color_planes_cvec"])]
    return steps


def grid_failing(case):
    from parmgmc_amd.capi import lib
    from parmgmc_amd.wrappers import _ptr, _stream

    return [Failing("null_b", lambda g, x: lib.pmg_grid_apply(g._h, None, _ptr(x["y"].clone()), _stream()), ARG_NULL),
            Failing("sweep_type_7", lambda g, x: status(lambda: g.set_sweep_type(7)), SUP),
            Failing("colour_2", lambda g, x: status(lambda: g.sweep_color_cvec(2, x["bc"], x["yc"].clone())), ARG_OUTOFRANGE),
            Failing("its_negative", lambda g, x: status(lambda: g.sample_cvec(x["bc"], x["yc"].clone(), -1, seed=1)), ARG_OUTOFRANGE),
            Failing("planes_outside", lambda g, x: status(lambda: g.sweep_color_planes_cvec(0, 1, g.nz, x["bc"], x["yc"].clone())), ARG_OUTOFRANGE)]


# ---- MCSOR --------------------------------------------------------------------------------------------------------------------
MCSOR_COMPACT = {"lap6x5x4_compact3": "lap6x5x4"}  # a row-compact update on one of MCSOR_CASES
MCSOR_ALL = list(SC.MCSOR_CASES) + list(MCSOR_COMPACT)


def _mcsor_lowrank(case):
    if case in MCSOR_COMPACT:
        n = SC.MCSOR_CASES[MCSOR_COMPACT[case]][0]().n
        return clustered(n, [[0, 1], [n // 2, n // 2 + 1], [n - 2, n - 1]], 36)
    mk, form = SC.MCSOR_CASES[case]
    return SC.observations(mk().n, 3, form, 31) if form else None  # what make_mcsor sets


def build_mcsor(case):
    """(A, mc)"""
    if case not in MCSOR_COMPACT:
        return SC.make_mcsor(case)
    A, mc = SC.make_mcsor(MCSOR_COMPACT[case])
    mc.set_lowrank(*_mcsor_lowrank(case))
    return A, mc


def mcsor_inputs(case):
    A, mc = build_mcsor(case)
    x = SC.chains_inputs(A.n, np.random.default_rng(1))
    lr = _mcsor_lowrank(case)
    if lr is not None:
        x["b_special"] = special_rows(x["b"], lr[0])
    pos, ld = mc.get_layout(), mc.layout_len()
    for k in ("b", "y") + (("b_special",) if lr is not None else ()):
        kl = k.replace("b", "bl", 1) if k != "y" else "yl"
        x[kl] = np.zeros(ld)
        x[kl][pos] = x[k]
    x = SC.to_dev(x)
    x["lowrank"] = lr
    return x


def _chains(tag, c, seeds, its=2, counter0=5, rhs=False, **kw):
    """a step: sample_chains on C chains with the shared b or one right-hand side per chain"""

    def fn(h, x):
        Y = x[f"Y{c}"].clone()
        return {tag + "_ctr": h.sample_chains(x[f"B{c}" if rhs else "b"], Y, its, seeds, counter0=counter0, **kw), tag: Y}

    return fn


def _mcsor_apply(mc, x):
    y = x["y"].clone()
    mc.apply(x["b"], y)
    return {"apply": y}


def _mcsor_sample(mc, x):
    y = x["y"].clone()
    return {"sample_ctr": mc.sample(x["b"], y, 2, seed=0xBEEF, counter0=3), "sample": y}


def _mcsor_residual(mc, x):
    r = zeros(mc.n)
    mc.residual(x["b"], x["y"], r)
    return {"residual": r}


def _mcsor_apply_chains(mc, x):
    Y = x["Y3"].clone()
    mc.apply_chains(x["b"], Y)
    return {"apply_chains": Y}


def _mcsor_layout(name):
    def fn(mc, x):
        from parmgmc_amd.capi import check, lib
        from parmgmc_amd.wrappers import _ptr, _stream

        h, s, out = mc._h, _stream(), {}
        if name == "to_layout":
            out["to_layout"] = zeros(mc.layout_len())
            check(lib.pmg_mcsor_to_layout(h, _ptr(x["b"]), _ptr(out["to_layout"]), s))
            out["from_layout"] = zeros(mc.n)
            check(lib.pmg_mcsor_from_layout(h, _ptr(x["yl"]), _ptr(out["from_layout"]), s))
        elif name == "apply_layout":
            out[name] = x["yl"].clone()
            check(lib.pmg_mcsor_apply_layout(h, _ptr(x["bl"]), _ptr(out[name]), s))
        elif name == "sample_layout":
            import ctypes

            out[name], ctr = x["yl"].clone(), ctypes.c_uint64()
            check(lib.pmg_mcsor_sample_layout(h, _ptr(x["bl"]), _ptr(out[name]), 2, 1, 0xBEEF, 9, ctypes.byref(ctr), s))
            out[name + "_ctr"] = ctr.value
        else:
            out[name] = zeros(mc.layout_len())
            check(lib.pmg_mcsor_residual_layout(h, _ptr(x["bl"]), _ptr(x["yl"]), _ptr(out[name]), s))
        return out

    return fn


def _mcsor_colour_sweeps(mc, x):
    y = x["yl"].clone()
    for colour in range(mc.get_num_colors()):
        mc.sweep_color_layout(colour, x["bl"], y, noisy=True, scaled=True, seed=0xD00D, counter=4)
    return {"colour_sweeps": y}


def mcsor_steps(case):
    sc = ["MCSOR.sample_chains"]
    steps = [Step("apply", _mcsor_apply, ["b", "y"], ["MCSOR.apply"]), Step("sample", _mcsor_sample, ["b", "y"], ["MCSOR.sample"]), Step("residual", _mcsor_residual, ["b", "y"], ["MCSOR.residual"]),
             Step("to_layout", _mcsor_layout("to_layout"), ["b", "yl"], []), Step("apply_layout", _mcsor_layout("apply_layout"), ["bl", "yl"], []),
             Step("sample_layout", _mcsor_layout("sample_layout"), ["bl", "yl"], []), Step("residual_layout", _mcsor_layout("residual_layout"), ["bl", "yl"], []),
             Step("chains3", _chains("chains3", 3, SEEDS[:3]), ["b", "Y3"], sc), Step("chains65", _chains("chains65", 65, SEEDS[:65]), ["b", "Y65"], sc),
             Step("chains3_reseeded", _chains("chains3_reseeded", 3, SEEDS[70:73]), ["b", "Y3"], sc),
             Step("chains_rhs3", _chains("chains_rhs3", 3, SEEDS[70:73], rhs=True), ["B3", "Y3"], sc), Step("chains_rhs65", _chains("chains_rhs65", 65, SEEDS[:65], rhs=True), ["B65", "Y65"], sc),
             Step("apply_chains", _mcsor_apply_chains, ["b", "Y3"], ["MCSOR.apply_chains"]), Step("sample_symmetric_omega1.3", _symmetric_omega(_mcsor_sample), ["b", "y"], ["MCSOR.sample"]),
             Step("chains3_symmetric_omega1.3", _symmetric_omega(_chains("chains3_symmetric", 3, SEEDS[:3])), ["b", "Y3"], sc)]
    if _mcsor_lowrank(case) is not None:
        steps += [Step("sample_special", _special(_mcsor_sample, b="b_special"), ["b_special", "y"], ["MCSOR.sample"]),
                  Step("sample_layout_special", _special(_mcsor_layout("sample_layout"), bl="bl_special"), ["bl_special", "yl"], []),
                  Step("chains3_special", _special(_chains("chains3", 3, SEEDS[:3]), b="b_special"), ["b_special", "Y3"], sc)]
    if _mcsor_lowrank(case) is None:  # the per-colour sweeps do not carry the low-rank repair
        steps.append(Step("colour_sweeps", _mcsor_colour_sweeps, ["bl", "yl"], ["MCSOR.sweep_color_layout"]))
    return steps


def _seed_array(c):
    return np.ascontiguousarray(SEEDS[:c], np.uint64)


def mcsor_failing(case):
    from parmgmc_amd.capi import lib
    from parmgmc_amd.wrappers import _ptr, _stream

    return [Failing("nchains_0", lambda mc, x: lib.pmg_mcsor_sample_chains(mc._h, 0, _seed_array(3).ctypes.data, _ptr(x["b"]), _ptr(x["Y3"].clone()), 1, 1, 0, None, _stream()), ARG_OUTOFRANGE),
            Failing("null_b", lambda mc, x: lib.pmg_mcsor_sample(mc._h, None, _ptr(x["y"].clone()), 1, 1, 1, 0, None, _stream()), ARG_NULL),
            Failing("sweep_type_7", lambda mc, x: status(lambda: mc.set_sweep_type(7)), SUP),
            Failing("colour_out_of_range", lambda mc, x: status(lambda: mc.sweep_color_layout(mc.get_num_colors(), x["bl"], x["yl"].clone())), ARG_OUTOFRANGE),
            Failing("null_b_chains", lambda mc, x: lib.pmg_mcsor_sample_chains(mc._h, 3, _seed_array(3).ctypes.data, None, _ptr(x["Y3"].clone()), 1, 1, 0, None, _stream()), ARG_NULL),
            Failing("its_negative", lambda mc, x: status(lambda: mc.sample_chains(x["b"], x["Y3"].clone(), -1, SEEDS[:3])), ARG_OUTOFRANGE)]


# ---- CholSampler --------------------------------------------------------------------------------------------------------------
def build_chol(case):
    from parmgmc_amd import CholSampler

    A = SC.MCSOR_CASES[case][0]()
    return CholSampler(A.rowptr, A.colidx, A.vals)


def chol_inputs(case):
    n = SC.MCSOR_CASES[case][0]().n
    rng = np.random.default_rng(3)
    return SC.to_dev({"b": rng.standard_normal(n), "y": rng.standard_normal(n)})


def _chol(tag, noisy, seed=5, counter=2, rhs="b"):
    def fn(ch, x):
        y = x["y"].clone()
        ch.sample(x[rhs], y, seed=seed, counter=counter, noisy=noisy)
        return {tag: y}

    return fn


def chol_steps(case):
    return [Step("sample", _chol("sample", True), ["b"], ["CholSampler.sample"]), Step("mean", _chol("mean", False), ["b"], ["CholSampler.sample"]),
            Step("sample_other_stream", _chol("sample_other_stream", True, seed=6, counter=9), ["b"], ["CholSampler.sample"]), Step("mean_of_y", _chol("mean_of_y", False, rhs="y"), ["y"], ["CholSampler.sample"])]


def chol_failing(case):
    from parmgmc_amd.capi import lib
    from parmgmc_amd.wrappers import _ptr, _stream

    return [Failing("null_b", lambda ch, x: lib.pmg_chol_sample(ch._h, None, _ptr(x["y"].clone()), 1, 5, 2, _stream()), ARG_NULL),
            Failing("null_y", lambda ch, x: lib.pmg_chol_sample(ch._h, _ptr(x["b"]), None, 1, 5, 2, _stream()), ARG_NULL)]


# ---- MGMC on a DMDA hierarchy ---------------------------------------------------------------------------------------------------
BALLS, WIDE = "33x17x17_L3_balls", "17x9x9_L3_wide3"  # a row-compact update (ball observations) and one kept dense on every level
GEO_LOWRANK = (BALLS, WIDE)
GEO_CASES = list(SC.GEO) + [BALLS, WIDE]


def _balls():
    import test_lrc

    return test_lrc.ball_matrix((33, 17, 17), [(0.3, 0.3, 0.4), (0.7, 0.6, 0.5), (0.5, 0.2, 0.8)], [0.12, 0.15, 0.1]), np.array([50.0, 80.0, 30.0])


def build_geo(case):
    from parmgmc_amd import MGMC

    if case == WIDE:
        mg = MGMC(17, 9, 9, 2.0, 3)
        mg.set_lowrank(*SC.observations(17 * 9 * 9, 3, "wide", 37))
        return mg.setup()
    if case != BALLS:
        return SC.make_geo(case)
    mg = MGMC(33, 17, 17, 2.0, 3)  # as test_device_mgmc_lrc_row_compact_form (tests/test_lrc.py) builds it
    mg.set_smoother(True, 1.1, 3, 1)
    mg.set_lowrank(*_balls())
    return mg.setup()


def geo_inputs(case):
    import torch

    mg = build_geo(case)
    rng = np.random.default_rng(4)
    b = rng.standard_normal(mg.n)
    x = SC.to_dev({"b": b, "y": rng.standard_normal(mg.n), "Y3": rng.standard_normal((mg.n, 3))})
    if case in GEO_LOWRANK:
        x["b_special"] = SC.dev(special_rows(b, _balls()[0] if case == BALLS else SC.observations(mg.n, 3, "wide", 37)[0]))
    gen, keep, top = torch.Generator(device="cuda").manual_seed(11), [], mg.levels - 1
    for name, level in (("top", top), ("below", top - 1)):
        x[name + "_b"], x[name + "_v"], x[name + "_e"] = SC._level_vec(mg, level, keep, gen), SC._level_vec(mg, level, keep, gen), SC._level_vec(mg, level - 1, keep, gen)
    torch.cuda.synchronize()
    return x


def _mg_sample(tag, its, seed, counter0, **kw):
    def fn(mg, x):
        y = x["y"].clone()
        return {tag + "_ctr": mg.sample(x["b"], y, its, seed=seed, counter0=counter0, **kw), tag: y}

    return fn


def _mg_callback(mg, x):
    y, seen = x["y"].clone(), []
    mg.sample(x["b"], y, 3, seed=8, callback=lambda it, yy: seen.append(yy.clone()))
    assert len(seen) == 3
    return {"callback": y, **{f"callback_sample{i}": s for i, s in enumerate(seen)}}


def _mg_setting(setter, on, off, call):
    def fn(mg, x):
        getattr(mg, setter)(on)
        try:
            return call(mg, x)
        finally:
            getattr(mg, setter)(off)

    return fn


def _level(mg, where):
    return mg.levels - 1 if where == "top" else mg.levels - 2


def _geo_level(where, op):
    def fn(mg, x):
        level, b, v = _level(mg, where), x[where + "_b"], x[where + "_v"]
        ldc = mg.level_layout(level - 1)[1]
        if op.startswith("sweep"):  # class-stencil levels only
            kw = {"sweep_forward": {}, "sweep_backward": {"backward": True}, "sweep_noisy": {"noisy": True, "seed": 0xBEEF, "counter": 3}}[op]
            out = v.clone()
            return {op: or_not_supported(lambda: mg.level_sweep(level, b, out, **kw) or out)}
        if op == "residual":
            out = zeros(v.numel())
            mg.level_residual(level, b, v, out)
        elif op == "restrict":
            out = zeros(ldc)
            mg.level_restrict(level, b.clone(), out)
        elif op == "residual_restrict":  # PMG_ERR_SUP where the cycle runs the two steps on this level
            out = zeros(ldc)
            return {op: or_not_supported(lambda: mg.level_residual_restrict(level, b, v, out) or out)}
        elif op == "prolong_add":
            out = v.clone()
            mg.level_prolong_add(level, x[where + "_e"], out)
        elif op.startswith("lowrank_post"):
            out = v.clone()
            mg.level_lowrank_post(level, out, backward=op.endswith("backward"))
        else:
            restricted = op.endswith("restricted")
            out = x[where + "_e"].clone() if restricted else b.clone()
            if restricted:  # PMG_ERR_ARG_WRONGSTATE above a level without an update of its own (the exact coarse sampler factors the sum)
                return {op: or_not_supported(lambda: mg.level_lowrank_residual_sub(level, v, out, restricted=True) or out, ARG_WRONGSTATE)}
            mg.level_lowrank_residual_sub(level, v, out)
        return {op: out}

    return fn


def _geo_chains(mg, x):
    Y = x["Y3"].clone()
    return {"sample_chains": or_not_supported(lambda: mg.sample_chains(x["b"], Y, 1, SEEDS[:3]))}  # DMDA hierarchies: PMG_ERR_SUP is the result


def geo_steps(case):
    s, bv = ["MGMC.sample"], lambda w: [w + "_b", w + "_v"]
    steps = [Step("sample", _mg_sample("sample", 2, 7, 1), ["b", "y"], s), Step("guesszero", _mg_sample("guesszero", 2, 7, 3, guesszero=True), ["b", "y"], s), Step("callback", _mg_callback, ["b", "y"], s),
             Step("correction_form", _mg_setting("set_correction_form", True, False, _mg_sample("literal", 2, 7, 1)), ["b", "y"], s),
             Step("unfused_transfers", _mg_setting("set_fused_transfers", False, True, _mg_sample("unfused", 2, 7, 1)), ["b", "y"], s),
             Step("sample_chains", _geo_chains, ["b", "Y3"], ["MGMC.sample_chains"])]
    ops = ["sweep_forward", "sweep_backward", "sweep_noisy", "residual", "restrict", "residual_restrict", "prolong_add"]
    if case in GEO_LOWRANK:
        steps.append(Step("sample_special", _special(_mg_sample("sample", 2, 7, 1), b="b_special"), ["b_special", "y"], s))
        ops += ["lowrank_post_forward", "lowrank_post_backward", "lowrank_residual_sub", "lowrank_residual_sub_restricted"]
    for where in ("top", "below"):
        for op in ops:
            method = next(m for m in ("sweep", "residual_restrict", "residual", "restrict", "prolong_add", "lowrank_post", "lowrank_residual_sub") if op.startswith(m))
            steps.append(Step(f"{where}_{op}", _geo_level(where, op), bv(where) + [where + "_e"], ["MGMC.level_" + method]))
    return steps


def mgmc_failing(hierarchy):
    """the refused calls of both MGMC kinds; hierarchy: the chains entry points exist (their nchains check comes first either way)"""

    def make(case):
        from parmgmc_amd.capi import lib
        from parmgmc_amd.wrappers import _ptr, _stream

        refusing = "top" if hierarchy else "below"  # a sliced-ELL or class-stencil level: the fused step is the grid level's
        vec = (lambda x: (x["lb"], x["lx"], x["lb"])) if hierarchy else (lambda x: (x["below_b"], x["below_v"], x["below_e"]))
        return [Failing("nchains_0", lambda mg, x: lib.pmg_mgmc_sample_chains(mg._h, 0, _seed_array(3).ctypes.data, _ptr(x["b"]), _ptr(x["Y3"].clone()), 1, 0, 0, None, None, None, _stream()), ARG_OUTOFRANGE),
                Failing("null_b", lambda mg, x: lib.pmg_mgmc_sample(mg._h, None, _ptr(x["y"].clone()), 1, 0, 7, 0, None, None, None, _stream()), ARG_NULL),
                Failing("level_out_of_range", lambda mg, x: status(lambda: mg.level_residual(mg.levels, vec(x)[0], vec(x)[1], vec(x)[0].clone())), ARG_OUTOFRANGE),
                Failing("set_smoother_its_0", lambda mg, x: status(lambda: mg.set_smoother(True, 1.0, 1, 0)), ARG_WRONGSTATE),
                Failing("residual_restrict_refused", lambda mg, x: status(lambda: mg.level_residual_restrict(_level(mg, refusing), vec(x)[0], vec(x)[1], zeros(mg.level_layout(_level(mg, refusing) - 1)[1]))), SUP),
                Failing("its_negative", lambda mg, x: status(lambda: mg.sample(x["b"], x["y"].clone(), -1, seed=7)), ARG_OUTOFRANGE)]

    return make


# ---- MGMC on an AIJ hierarchy ---------------------------------------------------------------------------------------------------
AIJ_CASES = {"chol": ("cholsampler", False), "gibbs": ("gibbs", False), "chol_k3": ("cholsampler", True), "gibbs_k3": ("gibbs", True)}


def _aij_lowrank(hier):
    n = len(hier[0][-1][0]) - 1
    return clustered(n, [np.arange(r, r + 3) for r in (5, n // 2, n - 8)], 33)  # row-compact on the fine level (test_alone asserts it)


def build_aij(case, hier):
    from parmgmc_amd import COLORING_ITERATED, MGMC

    coarse, lowrank = AIJ_CASES[case]
    if not lowrank:
        return SC.make_aij_mgmc(hier, coarse)
    mg = MGMC.from_hierarchy(*hier)  # make_aij_mgmc with the update set before set-up
    mg.set_coloring(COLORING_ITERATED)
    mg.set_smoother(True, 1.0, 1, 1)
    mg.set_coarse(coarse, 1)
    mg.set_lowrank(*_aij_lowrank(hier))
    return mg.setup()


def aij_inputs(case, hier):
    import torch

    mg = build_aij(case, hier)
    x = SC.chains_inputs(mg.n, np.random.default_rng(5))
    if AIJ_CASES[case][1]:
        x["b_special"] = special_rows(x["b"], _aij_lowrank(hier)[0])
    x = SC.to_dev(x)
    top = mg.levels - 1
    ld, ldc = mg.level_layout(top)[1], mg.level_layout(top - 1)[1]  # any vectors of the level's length serve
    x["lb"], x["lx"], x["le"] = zeros(ld), zeros(ld), zeros(ldc)
    x["lb"][: mg.n], x["lx"][: mg.n], x["le"][: min(ldc, mg.n)] = x["b"], x["y"], x["y"][: min(ldc, mg.n)]
    torch.cuda.synchronize()
    return x


def _aij_callback(mg, x):
    Y, seen = x["Y3"].clone(), []
    mg.sample_chains(x["b"], Y, 2, SEEDS[70:73], callback=lambda it, YY: seen.append(YY.clone()))
    assert len(seen) == 2
    return {"callback": Y, **{f"callback_sample{i}": s for i, s in enumerate(seen)}}


def _aij_level(op):
    def fn(mg, x):
        top = mg.levels - 1
        if op == "residual":
            out = zeros(x["lb"].numel())
            mg.level_residual(top, x["lb"], x["lx"], out)
        elif op == "restrict":
            out = zeros(x["le"].numel())
            mg.level_restrict(top, x["lb"].clone(), out)
        else:
            out = x["lx"].clone()
            mg.level_prolong_add(top, x["le"], out)
        return {"level_" + op: out}

    return fn


def aij_steps(case):
    sc = ["MGMC.sample_chains"]
    special = [Step("sample_special", _special(_mg_sample("sample", 2, SEEDS[1], 3), b="b_special"), ["b_special", "y"], ["MGMC.sample"]),
               Step("chains3_special", _special(_chains("chains3", 3, SEEDS[:3], counter0=3), b="b_special"), ["b_special", "Y3"], sc)]
    return (special if AIJ_CASES[case][1] else []) + [Step("chains3", _chains("chains3", 3, SEEDS[:3], counter0=3), ["b", "Y3"], sc), Step("chains65", _chains("chains65", 65, SEEDS[:65], counter0=3), ["b", "Y65"], sc),
            Step("chains3_reseeded", _chains("chains3_reseeded", 3, SEEDS[70:73], counter0=3), ["b", "Y3"], sc),
            Step("chains_rhs3_guesszero", _chains("chains_rhs3", 3, SEEDS[70:73], its=1, counter0=3, rhs=True, guesszero=True), ["B3", "Y3"], sc),
            Step("chains_rhs65_guesszero", _chains("chains_rhs65", 65, SEEDS[:65], its=1, counter0=3, rhs=True, guesszero=True), ["B65", "Y65"], sc),
            Step("correction_form", _mg_setting("set_correction_form", True, False, _chains("literal", 3, SEEDS[70:73], counter0=1)), ["b", "Y3"], sc),
            Step("callback", _aij_callback, ["b", "Y3"], sc), Step("sample", _mg_sample("sample", 2, SEEDS[1], 3), ["b", "y"], ["MGMC.sample"]),
            Step("level_residual", _aij_level("residual"), ["lb", "lx"], ["MGMC.level_residual"]), Step("level_restrict", _aij_level("restrict"), ["lb"], ["MGMC.level_restrict"]),
            Step("level_prolong_add", _aij_level("prolong_add"), ["le", "lx"], ["MGMC.level_prolong_add"])]


# ---- WoodburySampler: the handle is (A, mc, wb, state) of make_woodbury ---------------------------------------------------------
def build_woodbury(case):
    state = {}
    return SC.make_woodbury(state) + (state,)


def woodbury_inputs(case):
    return SC.to_dev(SC.chains_inputs(120, np.random.default_rng(6)))


def _wb_chains(tag, c, seeds):
    def fn(w, x):
        w[3]["seeds"] = seeds
        Y = x[f"Y{c}"].clone()
        return {tag + "_ctr": w[2].run_chains(x["b"], Y, 2, seeds, counter0=2), tag: Y}

    return fn


def _wb_run(w, x):
    w[3]["seed"] = SEEDS[4]
    y = x["y"].clone()
    return {"run_ctr": w[2].run(x["b"], y, 2, SEEDS[4], counter0=2), "run": y}


def woodbury_steps(case):
    rc = ["WoodburySampler.run_chains", "MCSOR.sample_chains"]
    return [Step("run", _wb_run, ["b", "y"], ["WoodburySampler.run", "MCSOR.sample"]), Step("chains3", _wb_chains("chains3", 3, SEEDS[:3]), ["b", "Y3"], rc),
            Step("chains65", _wb_chains("chains65", 65, SEEDS[:65]), ["b", "Y65"], rc), Step("chains3_reseeded", _wb_chains("chains3_reseeded", 3, SEEDS[70:73]), ["b", "Y3"], rc)]


def woodbury_failing(case):
    from parmgmc_amd.capi import lib
    from parmgmc_amd.wrappers import _ptr, _stream

    return [Failing("nchains_0", lambda w, x: lib.pmg_woodbury_noisy_rhs_chains(w[2]._h, 0, _seed_array(3).ctypes.data, 0, _ptr(x["b"]), _ptr(x["Y3"].clone()), _stream()), ARG_OUTOFRANGE),
            Failing("null_b", lambda w, x: lib.pmg_woodbury_noisy_rhs(w[2]._h, None, _ptr(x["y"].clone()), 1, 0, _stream()), ARG_NULL),
            Failing("inner_sweep_type_7", lambda w, x: status(lambda: w[1].set_sweep_type(7)), SUP)]


# ---- PC layer: the handle is (pc, inner PCs whose counters the step sets too) ---------------------------------------------------
PC_TYPES = ["mcgibbs", "sorgibbs", "cholsampler", "gamgmc", "woodbury", "parsor"]


def build_pc(case):
    import oracle as O
    from parmgmc_amd import pc as P

    P.initialize()
    P.options_clear()
    try:
        A = O.shifted_laplace(9, 9, 1, 10.0)  # the 9 x 9 ex1 operator
        csr = P.Mat.csr(A.rowptr, A.colidx, A.vals)
        pc, inner = P.PC(case), []
        if case == "gamgmc":
            for k, v in SC.PC_TYPES["gamgmc"].items():
                P.options_set_value(k, v)
        if case == "woodbury":  # the sampler is handed over, so that its counter can be set (the set-up destroys the solver)
            inner = [P.PC("sorgibbs")]
            pc.woodbury_set_sampler(inner[0])
            pc.woodbury_set_solver(P.PC("parsor"))
            pc.set_operators(csr.lrc(*SC.observations(A.n, 3, "rows", 34)))
        elif case in ("cholsampler", "sorgibbs", "parsor"):  # need the assembled matrix
            pc.set_operators(csr)
        else:
            pc.set_operators(P.Mat.dmda(9, 9, 1, 10.0))
        pc.set_from_options()
        return pc, inner
    finally:
        P.options_clear()


def pc_inputs(case):
    rng = np.random.default_rng(7)
    return SC.to_dev({"b": rng.standard_normal(81), "y": rng.standard_normal(81)})


def pc_bracket(h, counter):
    """the global seed that gives this PC the stream PC_SEED whatever its creation index (seed of a PC = global seed + stride *
    (creation index + 1), include/parmgmc_hip.h), and the stated counter on it and on its inner PCs"""
    from parmgmc_amd import pc as P

    pc, inner = h
    P.set_seed(0)
    P.set_seed((PC_SEED - pc.noise_state()[0]) % 2**64)
    for p in [pc] + inner:
        p.set_noise_counter(counter)
    assert pc.noise_state() == (PC_SEED, counter)


def _pc(name, counter, call):
    def fn(h, x):
        pc_bracket(h, counter)
        y = x["y"].clone()
        out = {name: or_not_supported(lambda: call(h[0], x["b"], y) or y)}
        out[name + "_counters"] = tuple(p.noise_state()[1] for p in [h[0]] + h[1])
        return out

    return fn


def pc_steps(case):
    steps = [Step("apply_richardson", _pc("apply_richardson", 5, lambda pc, b, y: pc.apply_richardson(b, y, 2) and None), ["b"], ["PC.apply_richardson"]),
             Step("apply", _pc("apply", 9, lambda pc, b, y: pc.apply(b, y)), ["b"], ["PC.apply"]),
             Step("richardson_guesszero", _pc("richardson_guesszero", 2, lambda pc, b, y: pc.apply_richardson(b, y, 1, guesszero=True) and None), ["b"], ["PC.apply_richardson"]),
             Step("ksp_solve", _pc("ksp_solve", 0, lambda pc, b, y: pc.ksp_solve(b, y, 2, guess_nonzero=False)), ["b"], ["PC.ksp_solve"]),
             Step("ksp_solve_guess", _pc("ksp_solve_guess", 3, lambda pc, b, y: pc.ksp_solve(b, y, 2)), ["b"], ["PC.ksp_solve"])]
    if case == "parsor":
        steps.append(Step("parsor_apply_sor", _pc("parsor_apply_sor", 0, lambda pc, b, y: pc.parsor_apply_sor(b, 2, False, y)), ["b"], ["PC.parsor_apply_sor"]))
    return steps


def pc_failing(case):
    from parmgmc_amd.capi import lib
    from parmgmc_amd.wrappers import _ptr, _stream

    return [Failing("null_b", lambda h, x: lib.pmg_pc_apply(h[0]._h, None, _ptr(x["y"].clone()), _stream()), ARG_NULL),
            Failing("its_negative", lambda h, x: status(lambda: h[0].apply_richardson(x["b"], x["y"].clone(), -1)), ARG_OUTOFRANGE)]


# ---- ChainStats / ChainCov on the ex6 operator, C = 8 ---------------------------------------------------------------------------
NCHAINS, NSTEPS = 8, 3


def build_chainstats(case, ex6):
    from parmgmc_amd import ChainStats

    n = ex6[0].n
    return ChainStats(n, NCHAINS, [None, np.random.default_rng(9).standard_normal(n)], max_steps=NSTEPS + 1)


def build_chaincov(case, ex6):
    from parmgmc_amd.wrappers import ChainCov

    A = ex6[0]
    return ChainCov.from_csr(A.rowptr, A.colidx, A.vals, NCHAINS, max_steps=NSTEPS + 1)


def stats_inputs(case, ex6):
    rng = np.random.default_rng(8)
    return SC.to_dev({f"Y{i}": rng.standard_normal((ex6[0].n, NCHAINS)) for i in range(NSTEPS)})


def _stats_readout(cs, prefix=""):
    mean, var = cs.fields()
    out = {"mean": mean, "var": var, "count": cs.count(), "rhat0": cs.rhat(0), "rhat1": cs.rhat(1), "trace0": cs.trace(0), "trace1": cs.trace(1)}
    tau, window, valid = cs.iact_device(1)
    out.update(iact_tau=tau, iact_window=window, iact_valid=valid)
    return {prefix + k: v for k, v in out.items()}


def _stats(variant):
    def fn(cs, x):
        from parmgmc_amd.capi import check, lib
        from parmgmc_amd.wrappers import _stream

        cs.reset()
        if variant == "reset_in_between":  # other updates, forgotten
            cs.update(x["Y2"])
            cs.update(x["Y0"])
            _stats_readout(cs)
            cs.reset()
        if variant == "set_stream":
            check(lib.pmg_chainstats_set_stream(cs._h, _stream()))
        for i in range(NSTEPS):
            cs.update(x[f"Y{i}"])
            if variant == "readouts_between" and i:  # get_fields, get_trace, rhat, iact_device between the updates
                _stats_readout(cs)
        return _stats_readout(cs)

    return fn


STATS_VARIANTS = ["updates", "readouts_between", "reset_in_between", "set_stream"]


def chainstats_steps(case):
    calls = ["ChainStats.update", "ChainStats.reset", "ChainStats.fields", "ChainStats.trace", "ChainStats.rhat", "ChainStats.iact_device", "ChainStats.count"]
    return [Step(v, _stats(v), [f"Y{i}" for i in range(NSTEPS)], calls) for v in STATS_VARIANTS]


def chainstats_failing(case):
    from parmgmc_amd.capi import lib
    from parmgmc_amd.wrappers import _stream

    return [Failing("null_Y", lambda cs, x: lib.pmg_chainstats_update(cs._h, None, _stream()), ARG_NULL),
            Failing("qoi_out_of_range", lambda cs, x: status(lambda: cs.trace(2, 0, 0)), ARG_OUTOFRANGE),
            Failing("steps_out_of_range", lambda cs, x: status(lambda: cs.trace(0, 0, NSTEPS + 2)), ARG_OUTOFRANGE)]


def _cov(variant):
    def fn(cov, x):
        cov.reset()
        out = {}
        if variant == "reset_in_between":
            cov.update(x["Y2"])
            cov.errors()
            cov.reset()
        if variant == "covariance":  # records nothing
            out["covariance"] = cov.covariance(x["Y1"])
        for i in range(NSTEPS):
            cov.update(x[f"Y{i}"])
            if variant == "readouts_between":
                cov.errors()
                cov.covariance(x["Y2"])
        out.update(errors=cov.errors(), count=cov.count())
        return out

    return fn


COV_VARIANTS = ["updates", "readouts_between", "reset_in_between", "covariance"]


def chaincov_steps(case):
    calls = ["ChainCov.update", "ChainCov.reset", "ChainCov.errors", "ChainCov.count", "ChainCov.covariance"]
    return [Step(v, _cov(v), [f"Y{i}" for i in range(NSTEPS)], calls) for v in COV_VARIANTS]


def chaincov_failing(case):
    from parmgmc_amd.capi import lib
    from parmgmc_amd.wrappers import _stream

    return [Failing("null_Y", lambda cov, x: lib.pmg_chaincov_update(cov._h, None, _stream()), ARG_NULL),
            Failing("steps_out_of_range", lambda cov, x: status(lambda: cov.errors(0, NSTEPS + 2)), ARG_OUTOFRANGE)]


# ---- the catalogue --------------------------------------------------------------------------------------------------------------
# kind: (cases, build(case, ctx), inputs(case, ctx), steps(case), failing(case)); ctx = {"aij": ..., "ex6": ...}, the hierarchies
KINDS = {
    "grid": (list(GRID_CASES), lambda c, ctx: build_grid(c), lambda c, ctx: grid_inputs(c), grid_steps, grid_failing),
    "mcsor": (MCSOR_ALL, lambda c, ctx: build_mcsor(c)[1], lambda c, ctx: mcsor_inputs(c), mcsor_steps, mcsor_failing),
    "chol": (["lap6x5x4"], lambda c, ctx: build_chol(c), lambda c, ctx: chol_inputs(c), chol_steps, chol_failing),
    "mgmc_geo": (GEO_CASES, lambda c, ctx: build_geo(c), lambda c, ctx: geo_inputs(c), geo_steps, mgmc_failing(False)),
    "mgmc_aij": (list(AIJ_CASES), lambda c, ctx: build_aij(c, ctx["aij"]), lambda c, ctx: aij_inputs(c, ctx["aij"]), aij_steps, mgmc_failing(True)),
    "woodbury": (["lap6x5x4_k3"], lambda c, ctx: build_woodbury(c), lambda c, ctx: woodbury_inputs(c), woodbury_steps, woodbury_failing),
    "pc": (PC_TYPES, lambda c, ctx: build_pc(c), lambda c, ctx: pc_inputs(c), pc_steps, pc_failing),
    "chainstats": (["ex6"], lambda c, ctx: build_chainstats(c, ctx["ex6"]), lambda c, ctx: stats_inputs(c, ctx["ex6"]), chainstats_steps, chainstats_failing),
    "chaincov": (["ex6"], lambda c, ctx: build_chaincov(c, ctx["ex6"]), lambda c, ctx: stats_inputs(c, ctx["ex6"]), chaincov_steps, chaincov_failing),
}
LOWRANK_SUBJECTS = ([("grid", c) for c, v in GRID_CASES.items() if v[4] is not None] + [("mcsor", c) for c in MCSOR_ALL if _mcsor_lowrank(c) is not None]
                    + [("mgmc_geo", c) for c in GEO_LOWRANK] + [("mgmc_aij", c) for c, v in AIJ_CASES.items() if v[1]])
# the cases whose update must be in the row-compact form (the one that writes b in place); test_alone asserts it with the sizes queries
ROW_COMPACT = [("grid", "33x7x3_lines3"), ("grid", "pair256x9x5_lines3"), ("mcsor", "lap6x5x4_compact3"), ("mgmc_geo", BALLS), ("mgmc_aij", "chol_k3"), ("mgmc_aij", "gibbs_k3")]


def subjects():
    return [(kind, case) for kind, v in KINDS.items() for case in v[0]]


def subject(kind, case, ctx):
    cases, build, inputs, steps, failing = KINDS[kind]
    assert case in cases
    return Subject(kind, case, lambda: build(case, ctx), lambda: inputs(case, ctx), steps(case), failing(case))


# methods of parmgmc_amd/wrappers.py that take device vectors and are in no step, with the reason
EXCLUDED = {
    "WoodburySampler.correction": "reads the correction back to the host; takes no device vector",
    "ChainStats.iact": "host arithmetic on ChainStats.trace, which the steps read",
    "ChainStats.set_qoi": "construction: the weights are part of how the object was built",
}
