"""Every option key and setter of the PC layer (parmgmc_amd/csrc/pmg_pc.c) with the sampler it selects IN THE REFERENCE.

A helper, not collected by pytest.  CASES is one table; every entry names a PC type, an operator, the option keys and
setter calls to apply, and the configuration the reference's own sources give for them -- written out by hand from the
lines cited beside each entry, never derived by calling into pmg_pc.c.  The builders at the end turn such a
configuration into the expected chain on the CPU oracle with the noise of a given (seed, counter).

Conventions the table relies on (the library's own, stated in include/parmgmc_hip.h):
  * a PC's noise counter counts DRAWS: a forward or backward Gibbs sample takes one, a symmetric one two
    (src/pc_mcgibbs.c:172-181 draws before each half sweep); gamgmc, cholsampler and woodbury take one per sample;
  * the reference's serial colouring is one colour (src/mc_sor.c:397-410) and its parallel one PETSc's; the colouring
    rules here (red-black on a DMDA, greedy / lexlevels / iterated on a CSR matrix) are this build's, so
    -pc_*_coloring has no reference line.
"""
from collections import namedtuple
from functools import lru_cache
from pathlib import Path

import numpy as np

import oracle as O
from mgmc_oracle import M64, LrcMgmcOracle, level_seed, oracle_chain, oracle_hierarchy

FWD, BWD, SYM = O.SOR_FORWARD, O.SOR_BACKWARD, O.SOR_SYMMETRIC
SUP, ARG_WRONG, OUTOFRANGE, WRONGSTATE, UNKNOWN_TYPE = 56, 62, 63, 73, 86
STREAM_STRIDE = 0xD1B54A32D192ED03  # seed of a PC = pmg_seed + STREAM_STRIDE * (creation index + 1)
ETA_TAG = 0x632BE59BD9B4E019  # stream of the low-rank noise term eta (tests/test_lrc.py)
NSAMPLES = 3

# what the reference runs: single-level Gibbs (scaled noise?, omega, sweep type, colouring rule of this build)
Gibbs = namedtuple("Gibbs", "scaled omega sweep coloring")
# PCGAMGMC: levels, sweeps per smoothing leg, the level sampler's (scaled, omega, sweep), coarse PC type and its sweeps
MG = namedtuple("MG", "levels nu scaled omega sweep coarse coarse_its")
Chol = namedtuple("Chol", "")
Parsor = namedtuple("Parsor", "omega its")
Woodbury = namedtuple("Woodbury", "sampler solver")
Shell = namedtuple("Shell", "sweep coloring")  # PCSHELL around MCSORApply: one deterministic sweep

Case = namedtuple("Case", "id pc op opts calls expect error prefix cite")


def case(id, pc, op, opts=None, calls=(), expect=None, error=None, prefix="", cite=""):
    """calls: (stage, C name of the setter, args); stage "pre" = before set_from_options, 0 = after it and before the first
    sample, 2 = between sample 2 and sample 3.  expect: one configuration, or one per sample.  error: (status, where)
    with where = "set_from_options" or the C name of the failing setter."""
    if expect is not None and not isinstance(expect, list):
        expect = [expect] * NSAMPLES
    return Case(id, pc, op, dict(opts or {}), tuple(calls), None if expect is None else tuple(expect), error, prefix, cite)


# ----------------------------------------------------------------------------------------------------------------
# operators and inputs
# ----------------------------------------------------------------------------------------------------------------
# (the ...b operators: another operator of the same size, for set-up after pmg_pc_set_operators)
DMDA_OPS = {"dmda9x9": (9, 9, 1, 10.0), "dmda6x5x4": (6, 5, 4, 2.0), "dmda9x9b": (9, 9, 1, 4.0)}
MG_OPS = {"mg9x9": (9, 9, 1, 2.0), "mg9x5x5": (9, 5, 5, 2.0), "mg17x9x9": (17, 9, 9, 2.0), "mg9x9lrc": (9, 9, 1, 2.0), "mg9x9b": (9, 9, 1, 3.0)}
CSR_OPS = ("csr7x6", "lshape", "csr9x9lrc", "csr7x6b")


def ball_observations(nx, ny, coords, radii, obsvals, sigma2):
    """the observation factors of tests/test_gpu_pc_layer.py (MakeObservationMats, reference src/obs.c:135-180)"""
    xs, ys = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny), indexing="xy")
    pts = np.stack([xs.ravel(), ys.ravel()], 1)
    h2 = 1.0 / ((nx - 1) * (ny - 1))
    B = np.zeros((nx * ny, len(radii)))
    for i, r in enumerate(radii):
        inside = ((pts - np.asarray(coords[2 * i:2 * i + 2])) ** 2).sum(1) < r * r
        B[inside, i] = h2 / (np.pi * r * r)
    S = np.full(len(radii), 1.0 / sigma2)
    return B, S, B @ (S * np.asarray(obsvals))


@lru_cache(maxsize=None)
def inputs(op):
    """dict(kind, A (O.CSR of the base matrix), grid, kappa, B, S, b, y0): everything a case on `op` runs on"""
    grid = kappa = B = S = None
    if op in DMDA_OPS or op in MG_OPS:
        *grid, kappa = (DMDA_OPS.get(op) or MG_OPS[op])
        grid = tuple(grid)
        A, kind = O.shifted_laplace(*grid, kappa), "dmda"
    elif op == "csr7x6":
        A, kind = O.shifted_laplace(7, 6, 1, 3.0), "csr"
    elif op == "csr7x6b":
        A, kind = O.shifted_laplace(7, 6, 1, 5.0), "csr"
    elif op == "csr9x9lrc":
        A, kind = O.shifted_laplace(9, 9, 1, 1.0), "csr"
    elif op == "lshape":  # the P1 matrix of the unrefined mesh: irregular rows, the three colourings differ
        from fem_p1 import assemble_p1, read_gmsh41_triangles

        xy, tris = read_gmsh41_triangles(Path(__file__).resolve().parent / "golden" / "lshape.msh")
        A, kind = O.CSR.from_scipy(assemble_p1(xy, tris, kappa=1.0)), "csr"
    else:
        raise KeyError(op)
    rng = np.random.default_rng(sorted(list(DMDA_OPS) + list(MG_OPS) + list(CSR_OPS)).index(op) + 100)
    b, y0 = rng.standard_normal(A.n), rng.standard_normal(A.n)
    if op.endswith("lrc"):  # rank 2, the two balls of test_woodbury_chain_matches_oracle_and_samples_the_posterior
        B, S, f = ball_observations(9, 9, [0.25, 0.25, 0.75, 0.75], [0.2, 0.2], [1.0, -1.0], 1e-3)
        b = b + f
    return dict(op=op, kind=kind, A=A, grid=grid, kappa=kappa, B=B, S=S, b=b, y0=y0)


# ----------------------------------------------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------------------------------------------
def _gibbs_cases():
    out = []
    mc, sg = "src/pc_mcgibbs.c", "src/pc_sorgibbs.c"
    for op, kind in [("dmda9x9", "dmda"), ("dmda6x5x4", "dmda"), ("csr7x6", "csr"), ("lshape", "csr")]:
        col = "redblack" if kind == "dmda" else "greedy"
        G = lambda scaled, omega, sweep, c=col: Gibbs(scaled, omega, sweep, c)  # noqa: E731
        t = f"-{op}"
        # --- mcgibbs: PCCreate :311-313 (omega 1, forward), scaled noise sqrt((2-omega)/omega) :150 ---
        out += [
            case("mcgibbs-default" + t, "mcgibbs", op, expect=G(True, 1.0, FWD), cite=f"{mc}:311-313"),
            case("mcgibbs-omega1.3" + t, "mcgibbs", op, {"-pc_mcgibbs_omega": "1.3"}, expect=G(True, 1.3, FWD), cite=f"{mc}:197"),
            case("mcgibbs-omega0.7" + t, "mcgibbs", op, {"-pc_mcgibbs_omega": "0.7"}, expect=G(True, 0.7, FWD), cite=f"{mc}:197"),
            case("mcgibbs-forward" + t, "mcgibbs", op, {"-pc_mcgibbs_forward": ""}, expect=G(True, 1.0, FWD), cite=f"{mc}:201-202"),
            case("mcgibbs-backward" + t, "mcgibbs", op, {"-pc_mcgibbs_backward": ""}, expect=G(True, 1.0, BWD), cite=f"{mc}:204-205"),
            case("mcgibbs-symmetric" + t, "mcgibbs", op, {"-pc_mcgibbs_symmetric": ""}, expect=G(True, 1.0, SYM), cite=f"{mc}:207-208"),
            case("mcgibbs-symmetric-omega0.7" + t, "mcgibbs", op, {"-pc_mcgibbs_symmetric": "", "-pc_mcgibbs_omega": "0.7"}, expect=G(True, 0.7, SYM), cite=f"{mc}:197,207-208"),
            # forward, backward, symmetric are tested in this order, each overwriting the type: symmetric wins
            case("mcgibbs-all-three-sweeps" + t, "mcgibbs", op, {"-pc_mcgibbs_forward": "", "-pc_mcgibbs_backward": "", "-pc_mcgibbs_symmetric": ""}, expect=G(True, 1.0, SYM), cite=f"{mc}:200-208"),
            # setters before the first sample: PCMulticolorGibbsSetOmega :271-279, SetSweepType :281-288
            case("mcgibbs-set-omega-first" + t, "mcgibbs", op, calls=[(0, "pmg_pc_mcgibbs_set_omega", (1.3,))], expect=G(True, 1.3, FWD), cite=f"{mc}:271-279"),
            case("mcgibbs-set-sweep-first" + t, "mcgibbs", op, calls=[(0, "pmg_pc_mcgibbs_set_sweep_type", (BWD,))], expect=G(True, 1.0, BWD), cite=f"{mc}:281-288"),
            # ... and between sample 2 and 3: the chain goes on from the old y with the new parameter
            case("mcgibbs-set-omega-mid" + t, "mcgibbs", op, calls=[(2, "pmg_pc_mcgibbs_set_omega", (0.7,))], expect=[G(True, 1.0, FWD)] * 2 + [G(True, 0.7, FWD)], cite=f"{mc}:165,271-279"),
            case("mcgibbs-set-sweep-mid" + t, "mcgibbs", op, {"-pc_mcgibbs_omega": "1.3"}, calls=[(2, "pmg_pc_mcgibbs_set_sweep_type", (SYM,))], expect=[G(True, 1.3, FWD)] * 2 + [G(True, 1.3, SYM)], cite=f"{mc}:281-288"),
            # --- sorgibbs: unscaled noise sqrt(diag), omega 1 (:82, :94), forward (:62) ---
            case("sorgibbs-default" + t, "sorgibbs", op, expect=G(False, 1.0, FWD), cite=f"{sg}:76-103"),
            case("sorgibbs-forward" + t, "sorgibbs", op, {"-pc_sorgibbs_forward": ""}, expect=G(False, 1.0, FWD), cite=f"{sg}:264-278"),
            case("sorgibbs-local-forward" + t, "sorgibbs", op, {"-pc_sorgibbs_local_forward": ""}, expect=G(False, 1.0, FWD), cite=f"{sg}:274 (= forward on one device)"),
            # a sorgibbs PC has no omega key: the mcgibbs one in the database is not its own
            case("sorgibbs-ignores-mcgibbs-omega" + t, "sorgibbs", op, {"-pc_mcgibbs_omega": "1.3", "-pc_mcgibbs_symmetric": ""}, expect=G(False, 1.0, FWD), cite=f"{sg}:264-278"),
        ]
        if kind == "csr":
            for pc, scaled in (("mcgibbs", True), ("sorgibbs", False)):
                # (a 5-point grid has two first-fit colours, where the iterated rule returns first-fit: only lshape tells them apart)
                for rule in ("greedy", "lexlevels") + (("iterated",) if op == "lshape" else ()):
                    out.append(case(f"{pc}-coloring-{rule}{t}", pc, op, {f"-pc_{pc}_coloring": rule}, expect=Gibbs(scaled, 1.0, FWD, rule), cite="this build's colouring rules (include/parmgmc_hip.h)"))
    # --- errors ---
    for op in ("dmda9x9", "csr7x6"):
        t = f"-{op}"
        out += [
            case("mcgibbs-coloring-unknown" + t, "mcgibbs", op, {"-pc_mcgibbs_coloring": "jp"}, error=(ARG_WRONG, "set_from_options")),
            case("sorgibbs-coloring-unknown" + t, "sorgibbs", op, {"-pc_sorgibbs_coloring": "jp"}, error=(ARG_WRONG, "set_from_options")),
            case("mcgibbs-omega-key-out-of-range" + t, "mcgibbs", op, {"-pc_mcgibbs_omega": "2.0"}, error=(OUTOFRANGE, "set_from_options"), cite=f"{mc}:197 PetscOptionsRangeReal(0, 2)"),
            case("mcgibbs-set-omega-out-of-range" + t, "mcgibbs", op, calls=[(0, "pmg_pc_mcgibbs_set_omega", (0.0,))], error=(OUTOFRANGE, "pmg_pc_mcgibbs_set_omega"), cite=f"{mc}:197"),
            case("mcgibbs-set-sweep-unsupported" + t, "mcgibbs", op, calls=[(0, "pmg_pc_mcgibbs_set_sweep_type", (4,))], error=(SUP, "pmg_pc_mcgibbs_set_sweep_type"), cite="src/mc_sor.c:427"),
            case("sorgibbs-rejects-set-omega" + t, "sorgibbs", op, calls=[(0, "pmg_pc_mcgibbs_set_omega", (1.3,))], error=(ARG_WRONG, "pmg_pc_mcgibbs_set_omega")),
            case("sorgibbs-rejects-set-sweep" + t, "sorgibbs", op, calls=[(0, "pmg_pc_mcgibbs_set_sweep_type", (BWD,))], error=(ARG_WRONG, "pmg_pc_mcgibbs_set_sweep_type")),
        ]
    return out


def _gamgmc_cases():
    """PCSetUp_GAMGMC injects the defaults (src/pc_gamgmc.c:318-342): levels sorgibbs x 1, coarse cholsampler x 1; PCMG's own
    default is 2 levels here (pmg_pc.c PCCreate_GAMGMC).  The level and the coarse sampler are real PCs of their type, so their
    keys mean what src/pc_mcgibbs.c:190-211 / src/pc_sorgibbs.c:264-278 say."""
    g, mc = "src/pc_gamgmc.c", "src/pc_mcgibbs.c"
    L = "-gamgmc_mg_levels_"
    C = "-gamgmc_mg_coarse_"
    D = MG(2, 1, False, 1.0, FWD, "cholsampler", 1)
    mcg = {L + "pc_type": "mcgibbs"}
    op = "mg9x9"
    out = [
        case("gamgmc-default", "gamgmc", op, expect=D, cite=f"{g}:318-342"),
        case("gamgmc-levels3", "gamgmc", op, {"-gamgmc_pc_mg_levels": "3"}, expect=D._replace(levels=3), cite="PCMG -pc_mg_levels"),
        case("gamgmc-set-levels3", "gamgmc", op, calls=[(0, "pmg_pc_gamgmc_set_levels", (3,))], expect=D._replace(levels=3), cite="include/parmgmc/pc/pc_gamgmc.h:15"),
        case("gamgmc-nu2", "gamgmc", op, {L + "ksp_max_it": "2"}, expect=D._replace(nu=2), cite=f"{g}:318-322"),
        case("gamgmc-levels-mcgibbs", "gamgmc", op, mcg, expect=D._replace(scaled=True), cite=f"{g}:330-334"),
        case("gamgmc-levels-sorgibbs", "gamgmc", op, {L + "pc_type": "sorgibbs"}, expect=D, cite=f"{g}:330-334"),
        case("gamgmc-levels-omega1.2", "gamgmc", op, {**mcg, L + "pc_mcgibbs_omega": "1.2"}, expect=D._replace(scaled=True, omega=1.2), cite=f"{mc}:197"),
        case("gamgmc-levels-forward", "gamgmc", op, {**mcg, L + "pc_mcgibbs_forward": ""}, expect=D._replace(scaled=True), cite=f"{mc}:201-202; examples/ex6.c:36"),
        case("gamgmc-levels-symmetric", "gamgmc", op, {**mcg, L + "pc_mcgibbs_symmetric": ""}, expect=D._replace(scaled=True, sweep=SYM), cite=f"{mc}:207-208"),
        case("gamgmc-levels-backward", "gamgmc", op, {**mcg, L + "pc_mcgibbs_backward": ""}, expect=D._replace(scaled=True, sweep=BWD), cite=f"{mc}:204-205"),
        # backward is tested before symmetric, so symmetric wins
        case("gamgmc-levels-symmetric-and-backward", "gamgmc", op, {**mcg, L + "pc_mcgibbs_symmetric": "", L + "pc_mcgibbs_backward": ""}, expect=D._replace(scaled=True, sweep=SYM), cite=f"{mc}:203-208"),
        # the level PC is sorgibbs: it has no mcgibbs keys
        case("gamgmc-levels-sorgibbs-ignores-omega", "gamgmc", op, {L + "pc_type": "sorgibbs", L + "pc_mcgibbs_omega": "1.2", L + "pc_mcgibbs_symmetric": ""}, expect=D, cite="src/pc_sorgibbs.c:264-278"),
        case("gamgmc-coarse-cholsampler", "gamgmc", op, {C + "pc_type": "cholsampler"}, expect=D, cite=f"{g}:336-342"),
        case("gamgmc-coarse-sorgibbs", "gamgmc", op, {C + "pc_type": "sorgibbs"}, expect=D._replace(coarse="sorgibbs"), cite="examples/ex4.c:28"),
        case("gamgmc-coarse-mcgibbs", "gamgmc", op, {C + "pc_type": "mcgibbs"}, expect=D._replace(coarse="mcgibbs"), cite="examples/ex4.c:31"),
        case("gamgmc-coarse-its3", "gamgmc", op, {C + "pc_type": "sorgibbs", C + "ksp_max_it": "3"}, expect=D._replace(coarse="sorgibbs", coarse_its=3), cite=f"{g}:324-328"),
        # On a cholsampler coarse PC the reference draws coarse_its exact samples and keeps the last (src/pc_chols.c:293-342):
        # each is independent of the one before, so the law is that of ONE draw, which is what the hierarchy makes.
        case("gamgmc-coarse-its3-cholsampler", "gamgmc", op, {C + "ksp_max_it": "3"}, expect=D._replace(coarse_its=3), cite="src/pc_chols.c:293-342"),
        case("gamgmc-ex1-line41", "gamgmc", op, {"-pc_gamgmc_mg_type": "mg", "-gamgmc_pc_mg_levels": "3", **mcg, C + "pc_type": "mcgibbs", C + "ksp_max_it": "2", L + "ksp_max_it": "2"},
             expect=MG(3, 2, True, 1.0, FWD, "mcgibbs", 2), cite="examples/ex1.c:41"),
        # coarse mcgibbs keys that ask for exactly what the hierarchy runs (the level sampler's omega and sweep) are accepted
        case("gamgmc-coarse-keys-match", "gamgmc", op, {**mcg, L + "pc_mcgibbs_omega": "1.2", L + "pc_mcgibbs_symmetric": "", C + "pc_type": "mcgibbs", C + "pc_mcgibbs_omega": "1.2", C + "pc_mcgibbs_forward": "", C + "pc_mcgibbs_backward": "", C + "pc_mcgibbs_symmetric": ""},
             expect=MG(2, 1, True, 1.2, SYM, "mcgibbs", 1), cite=f"{mc}:197-208 on the coarse PC"),
        case("gamgmc-9x5x5-default", "gamgmc", "mg9x5x5", expect=D, cite=f"{g}:318-342"),
        case("gamgmc-9x5x5-mcgibbs-backward-nu2", "gamgmc", "mg9x5x5", {**mcg, L + "pc_mcgibbs_backward": "", L + "ksp_max_it": "2", L + "pc_mcgibbs_omega": "0.8"}, expect=MG(2, 2, True, 0.8, BWD, "cholsampler", 1), cite=f"{mc}:197-205"),
        case("gamgmc-17x9x9-levels3", "gamgmc", "mg17x9x9", {"-gamgmc_pc_mg_levels": "3"}, expect=D._replace(levels=3), cite="PCMG -pc_mg_levels"),
        case("gamgmc-17x9x9-levels3-symmetric-omega1.2", "gamgmc", "mg17x9x9", {"-gamgmc_pc_mg_levels": "3", **mcg, L + "pc_mcgibbs_symmetric": "", L + "pc_mcgibbs_omega": "1.2", C + "pc_type": "mcgibbs", C + "pc_mcgibbs_omega": "1.2", C + "pc_mcgibbs_symmetric": "", C + "ksp_max_it": "2"},
             expect=MG(3, 1, True, 1.2, SYM, "mcgibbs", 2), cite=f"{mc}:197-208"),
        # MATLRC, rank 2 (src/pc_gamgmc.c:157-196)
        case("gamgmc-lrc-default", "gamgmc", "mg9x9lrc", {"-gamgmc_pc_mg_levels": "3"}, expect=D._replace(levels=3), cite=f"{g}:157-196"),
        case("gamgmc-lrc-mcgibbs-symmetric", "gamgmc", "mg9x9lrc", {"-gamgmc_pc_mg_levels": "3", **mcg, L + "pc_mcgibbs_symmetric": "", L + "pc_mcgibbs_omega": "1.2"}, expect=MG(3, 1, True, 1.2, SYM, "cholsampler", 1), cite=f"{g}:157-196"),
        # --- errors ---
        case("gamgmc-mg-type-gamg", "gamgmc", op, {"-pc_gamgmc_mg_type": "gamg"}, error=(SUP, "set_from_options"), cite=f"{g}:364 (GAMG aggregation is PETSc's)"),
        case("gamgmc-levels-omega-out-of-range", "gamgmc", op, {**mcg, L + "pc_mcgibbs_omega": "2.5"}, error=(OUTOFRANGE, "set_from_options"), cite=f"{mc}:197"),
        case("gamgmc-levels-type-unknown", "gamgmc", op, {L + "pc_type": "jacobi"}, error=(SUP, "set_from_options")),
        case("gamgmc-coarse-type-unknown", "gamgmc", op, {C + "pc_type": "lu"}, error=(SUP, "set_from_options")),
        # the coarse PC's own keys change the chain in the reference; the hierarchy cannot run them: an error naming the key
        case("gamgmc-coarse-omega-differs", "gamgmc", op, {C + "pc_type": "mcgibbs", C + "pc_mcgibbs_omega": "1.2"}, error=(SUP, "set_from_options"), cite=f"{mc}:197"),
        case("gamgmc-coarse-backward-differs", "gamgmc", op, {C + "pc_type": "mcgibbs", C + "pc_mcgibbs_backward": ""}, error=(SUP, "set_from_options"), cite=f"{mc}:204-205"),
        case("gamgmc-coarse-symmetric-differs", "gamgmc", op, {C + "pc_type": "mcgibbs", C + "pc_mcgibbs_symmetric": ""}, error=(SUP, "set_from_options"), cite=f"{mc}:207-208"),
        case("gamgmc-coarse-forward-differs", "gamgmc", op, {**mcg, L + "pc_mcgibbs_backward": "", C + "pc_type": "mcgibbs", C + "pc_mcgibbs_forward": ""}, error=(SUP, "set_from_options"), cite=f"{mc}:201-202"),
        # a coarse sorgibbs is omega 1 forward whatever the levels run
        case("gamgmc-coarse-sorgibbs-under-omega-levels", "gamgmc", op, {**mcg, L + "pc_mcgibbs_omega": "1.2", C + "pc_type": "sorgibbs"}, error=(SUP, "set_from_options"), cite="src/pc_sorgibbs.c:62,94"),
        case("gamgmc-set-levels-on-mcgibbs", "mcgibbs", "dmda9x9", calls=[(0, "pmg_pc_gamgmc_set_levels", (3,))], error=(ARG_WRONG, "pmg_pc_gamgmc_set_levels")),
    ]
    return out


WB_SAMPLER = Gibbs(True, 1.2, SYM, "greedy")
WB = Woodbury(WB_SAMPLER, Parsor(1.1, 1))
WB_KEYS = {"pc_woodbury_solver": "parsor", "pc_woodbury_sampler": "mcgibbs", "pc_woodbury_samplerpc_mcgibbs_symmetric": "", "pc_woodbury_samplerpc_mcgibbs_omega": "1.2", "pc_woodbury_solver_pc_parsor_omega": "1.1"}


def _other_cases():
    ch, ps, wb = "src/pc_chols.c", "src/pc_parsor.c", "src/woodbury.c"
    out = [
        case("cholsampler-csr7x6", "cholsampler", "csr7x6", expect=Chol(), cite=f"{ch}:262-342"),
        case("cholsampler-lrc", "cholsampler", "csr9x9lrc", expect=Chol(), cite=f"{ch}:119-153"),
        case("cholsampler-by-pc-type-key", "", "csr7x6", {"-pc_type": "cholsampler"}, expect=Chol(), cite="PCSetFromOptions -pc_type"),
        # parsor: PCCreate omega 1, its 1 (:1020-1039); idiag = omega / d (:69-81); lexicographic on one rank
        case("parsor-default", "parsor", "csr7x6", expect=Parsor(1.0, 1), cite=f"{ps}:880-890"),
        case("parsor-omega-key", "parsor", "lshape", {"-pc_parsor_omega": "1.3"}, expect=Parsor(1.3, 1), cite=f"{ps}:970-980"),
        case("parsor-its-key", "parsor", "csr7x6", {"-pc_parsor_its": "3"}, expect=Parsor(1.0, 3), cite=f"{ps}:970-980"),
        case("parsor-both-keys", "parsor", "lshape", {"-pc_parsor_omega": "0.8", "-pc_parsor_its": "2"}, expect=Parsor(0.8, 2), cite=f"{ps}:970-980"),
        case("parsor-set-omega", "parsor", "csr7x6", calls=[(0, "pmg_pc_parsor_set_omega", (1.3,))], expect=Parsor(1.3, 1), cite="include/parmgmc/pc/pc_parsor.h"),
        case("parsor-set-iterations", "parsor", "csr7x6", calls=[(0, "pmg_pc_parsor_set_iterations", (2,))], expect=Parsor(1.0, 2), cite="include/parmgmc/pc/pc_parsor.h"),
        # one rank owning every row sweeps in the lexicographic order (:703-878 with a single block)
        case("parsor-set-partition-one-rank", "parsor", "csr7x6", {"-pc_parsor_omega": "1.3"}, calls=[(0, "pmg_pc_parsor_set_partition", ([0, 42],))], expect=Parsor(1.3, 1), cite=f"{ps}:703-878"),
        case("parsor-set-omega-on-mcgibbs", "mcgibbs", "csr7x6", calls=[(0, "pmg_pc_parsor_set_omega", (1.3,))], error=(ARG_WRONG, "pmg_pc_parsor_set_omega")),
        case("parsor-set-iterations-on-mcgibbs", "mcgibbs", "csr7x6", calls=[(0, "pmg_pc_parsor_set_iterations", (2,))], error=(ARG_WRONG, "pmg_pc_parsor_set_iterations")),
        # woodbury: inner keys under <prefix>pc_woodbury_solver_ and <prefix>pc_woodbury_sampler (no underscore, :209)
        case("woodbury-keys", "woodbury", "csr9x9lrc", {"-" + k: v for k, v in WB_KEYS.items()}, expect=WB, cite=f"{wb}:187-257"),
        case("woodbury-keys-prefix-post", "woodbury", "csr9x9lrc", {"-post_" + k: v for k, v in WB_KEYS.items()}, expect=WB, prefix="post_", cite=f"{wb}:193-195,207-209"),
        # inner PCs handed over follow the same keys (PCWoodburySetSolver / SetSampler then PCSetFromOptions :254-255)
        case("woodbury-handed-over", "woodbury", "csr9x9lrc", {"-" + k: v for k, v in WB_KEYS.items() if k not in ("pc_woodbury_solver", "pc_woodbury_sampler")},
             calls=[("pre", "pmg_pc_woodbury_set_sampler", ("mcgibbs",)), ("pre", "pmg_pc_woodbury_set_solver", ("parsor",))], expect=WB, cite=f"{wb}:187-213,254-255"),
        case("woodbury-sorgibbs-lexlevels", "woodbury", "csr9x9lrc", {"-pc_woodbury_solver": "parsor", "-pc_woodbury_sampler": "sorgibbs", "-pc_woodbury_samplerpc_sorgibbs_coloring": "lexlevels"},
             expect=Woodbury(Gibbs(False, 1.0, FWD, "lexlevels"), Parsor(1.0, 1)), cite=f"{wb}:241-257"),
        case("woodbury-set-sampler-on-mcgibbs", "mcgibbs", "csr7x6", calls=[(0, "pmg_pc_woodbury_set_sampler", ("sorgibbs",))], error=(ARG_WRONG, "pmg_pc_woodbury_set_sampler")),
        case("woodbury-inner-type-unknown", "woodbury", "csr9x9lrc", {"-pc_woodbury_solver": "no_such_pc"}, error=(UNKNOWN_TYPE, "set_from_options")),
        # PCSHELL (examples/ex3.c:59-67): the apply routine and its context are the caller's
        case("shell-set-apply-and-context", "shell", "csr7x6", calls=[(0, "pmg_pc_shell_set_apply", ("mcsor_apply",)), (0, "pmg_pc_shell_set_context", (0x1234,))], expect=Shell(FWD, "greedy"), cite="examples/ex3.c:59-67,128-131"),
        case("shell-set-apply-on-mcgibbs", "mcgibbs", "csr7x6", calls=[(0, "pmg_pc_shell_set_apply", (None,))], error=(ARG_WRONG, "pmg_pc_shell_set_apply")),
        case("pc-type-key-unknown", "", "csr7x6", {"-pc_type": "no_such_pc"}, error=(UNKNOWN_TYPE, "set_from_options")),
    ]
    return out


CASES = _gibbs_cases() + _gamgmc_cases() + _other_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
CHAIN_CASES = [c for c in CASES if c.expect is not None and isinstance(c.expect[0], (Gibbs, MG, Chol, Woodbury)) and c.pc != "shell"]
PARSOR_CASES = [c for c in CASES if c.expect is not None and isinstance(c.expect[0], Parsor)]
ERROR_CASES = [c for c in CASES if c.error is not None]

# Pairs of cases whose configurations read differently but are ONE chain in the reference's arithmetic, for two reasons:
#   (1) the scaled noise factor sqrt((2 - omega) / omega) (src/pc_mcgibbs.c:150) is exactly 1 at omega = 1, so a mcgibbs PC at
#       omega 1 is a sorgibbs PC -- as a stand-alone PC, as level sampler and as coarse sampler;
#   (2) a cholsampler coarse PC iterated 3 times keeps the last of 3 independent exact draws: the law of one draw.
# test_pc_option_cases.py asserts every pair equal in the oracle; every other pair of cases on one operator and PC type with
# different configurations must differ by 1e-6.
_D = ["gamgmc-default", "gamgmc-levels-sorgibbs", "gamgmc-levels-sorgibbs-ignores-omega", "gamgmc-coarse-cholsampler"]  # one configuration
EQUAL_PAIRS = [
    # (1), stand-alone
    ("mcgibbs-default-dmda9x9", "sorgibbs-default-dmda9x9"),
    ("mcgibbs-default-dmda6x5x4", "sorgibbs-default-dmda6x5x4"),
    ("mcgibbs-default-csr7x6", "sorgibbs-default-csr7x6"),
    ("mcgibbs-default-lshape", "sorgibbs-default-lshape"),
    ("mcgibbs-forward-dmda9x9", "sorgibbs-forward-dmda9x9"),
    ("mcgibbs-coloring-lexlevels-lshape", "sorgibbs-coloring-lexlevels-lshape"),
    # (1), coarse mcgibbs vs coarse sorgibbs at omega 1 forward
    ("gamgmc-coarse-mcgibbs", "gamgmc-coarse-sorgibbs"),
    # (1), level mcgibbs at omega 1 forward vs level sorgibbs
    *[("gamgmc-levels-mcgibbs", d) for d in _D],
    *[("gamgmc-levels-forward", d) for d in _D],
    # (2)
    *[("gamgmc-coarse-its3-cholsampler", d) for d in _D],
    # (1) and (2)
    ("gamgmc-coarse-its3-cholsampler", "gamgmc-levels-mcgibbs"),
    ("gamgmc-coarse-its3-cholsampler", "gamgmc-levels-forward"),
]


# ----------------------------------------------------------------------------------------------------------------
# expected chains on the oracle
# ----------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def coloring(op, rule):
    inp = inputs(op)
    if rule == "redblack":
        return O.coloring_redblack(*inp["grid"])
    return {"greedy": O.coloring_greedy, "lexlevels": O.coloring_lexlevels, "iterated": O.coloring_iterated}[rule](inp["A"])


def draws_per_sample(cfg):
    return 2 if isinstance(cfg, Gibbs) and cfg.sweep == SYM else 1


def expected_gibbs(op, cfgs, seed, ctr0, y0, b=None):
    """PCApplyRichardson_MulticolorGibbs / _SORGibbs (src/pc_mcgibbs.c:155-188, src/pc_sorgibbs.c:115-134), one sample per
    configuration in cfgs; returns (samples, counter after them)"""
    inp = inputs(op)
    A, b = inp["A"], inp["b"] if b is None else b
    y, ctr, out = np.array(y0, copy=True), ctr0, []
    for cfg in cfgs:
        if inp["kind"] == "dmda":
            noise = lambda d, c=ctr: O.noise_grid(*inp["grid"], seed, c + d)  # noqa: E731
        else:
            noise = lambda d, c=ctr: O.noise_rows(A.n, seed, c + d)  # noqa: E731
        y = O.gibbs_samples(A, coloring(op, cfg.coloring), b, y, 1, noise, cfg.omega, cfg.sweep, cfg.scaled)
        ctr += draws_per_sample(cfg)
        out.append(y.copy())
    return out, ctr


@lru_cache(maxsize=None)
def _hierarchy(op, levels):
    inp = inputs(op)
    return oracle_hierarchy(*inp["grid"], inp["kappa"], levels)


def expected_mg(op, cfgs, seed, ctr0, y0, guesszero=False):
    """PCApplyRichardson_GAMGMC (src/pc_gamgmc.c:227-264); the coarse Gibbs PC of a valid case runs the level sampler's omega
    and sweep (anything else is an error case), and its noise scaling matters only at omega != 1, where it is mcgibbs's"""
    cfg = cfgs[0]
    assert all(c == cfg for c in cfgs)
    inp = inputs(op)
    n = len(cfgs)
    lv = _hierarchy(op, cfg.levels)
    coarse = "cholsampler" if cfg.coarse == "cholsampler" else "gibbs"
    if inp["B"] is None:
        return oracle_chain(inp["grid"], inp["kappa"], cfg.levels, inp["b"], y0, n, seed, ctr0, guesszero, nu=cfg.nu, scaled=cfg.scaled, omega=cfg.omega, sweep=cfg.sweep, coarse=coarse, coarse_its=cfg.coarse_its, lv=lv), ctr0 + n
    # MATLRC: the oracle's PCGAMGMC with per-level factors (src/pc_gamgmc.c:157-196)
    grid, k, top = inp["grid"], len(inp["S"]), cfg.levels - 1
    colors = [O.coloring_parity8(*x["dims"]) for x in lv]
    colors[top] = O.coloring_redblack(*grid)
    orc = LrcMgmcOracle(lv, colors, inp["B"], inp["S"], cfg.nu, cfg.omega, cfg.sweep, cfg.scaled, coarse, cfg.coarse_its)
    sizes = [x["A"].shape[0] for x in lv]
    y, out = np.array(y0, copy=True), []
    for it in range(n):
        s = ctr0 + it
        xi = lambda _it, l, c: O.noise_grid(*grid, level_seed(seed, l), 64 * s + c) if l == top else O.noise_rows(sizes[l], level_seed(seed, l), 64 * s + c)  # noqa: E731
        eta = lambda _it, l, c: O.noise_rows(k, (level_seed(seed, l) + ETA_TAG) & M64, 64 * s + c)  # noqa: E731
        y = orc.chain(inp["b"], y, 1, guesszero and it == 0, xi, eta, lambda _it: O.noise_rows(sizes[0], level_seed(seed, 0), 64 * s))
        out.append(y.copy())
    return out, ctr0 + n


@lru_cache(maxsize=None)
def _chol_factor(op):
    inp = inputs(op)
    M = inp["A"].dense()
    if inp["B"] is not None:
        M = M + inp["B"] @ np.diag(inp["S"]) @ inp["B"].T  # the explicit sum, src/pc_chols.c:119-153
    return O.potrf_lower(M)


def expected_chol(op, cfgs, seed, ctr0, y0=None):
    """PCApply_CholSampler per sample (src/pc_chols.c:262-342): independent of y"""
    inp = inputs(op)
    return [O.chol_sample(_chol_factor(op), inp["b"], O.noise_rows(inp["A"].n, seed, ctr0 + it)) for it in range(len(cfgs))], ctr0 + len(cfgs)


def lexicographic(A, b, x, omega, its):
    """PCPARSOR on one rank: lexicographic forward SOR with idiag = omega / d in one rounding (src/pc_parsor.c:69-81), as
    tests/test_parsor_partition.py builds it"""
    x = np.array(x, copy=True)
    dp = O.diag_pointers(A)
    idg = (1.0 / A.vals[dp]) if omega == 1.0 else omega / A.vals[dp]
    rows = np.arange(A.n, dtype=np.int32)
    for _ in range(its):
        O.lib().orc_parsor_rows(A.n, rows, A.rowptr, A.colidx, A.vals, dp, np.ascontiguousarray(idg), omega, np.ascontiguousarray(b), x, None, None, None, None)
    return x


def expected_parsor(op, cfg):
    """PCApply_PARSOR: its sweeps from a zero guess (src/pc_parsor.c:880-890)"""
    inp = inputs(op)
    return lexicographic(inp["A"], inp["b"], np.zeros(inp["A"].n), cfg.omega, cfg.its)


def expected_woodbury(op, cfgs, seed_w, ctr_w, seed_s, ctr_s, y0):
    """PCWOODBURY (src/woodbury.c:21-91, :263-289) as test_woodbury_chain_matches_oracle_and_samples_the_posterior builds it:
    C = solver(B) from a zero guess, G = C (S^-1 + B^T C)^-1; per sample w = b + B (sqrt|S| o xi), one sample of the inner
    sampler on w, y -= G (B^T y).  Returns (samples, outer counter, inner counter)."""
    cfg = cfgs[0]
    assert all(c == cfg for c in cfgs)
    inp = inputs(op)
    A, B, S, k = inp["A"], inp["B"], inp["S"], len(inp["S"])
    Cm = np.stack([lexicographic(A, B[:, c], np.zeros(A.n), cfg.solver.omega, cfg.solver.its) for c in range(k)], 1)
    G = Cm @ np.linalg.inv(np.diag(1.0 / S) + B.T @ Cm)
    sq = np.sqrt(np.abs(S))
    y, out = np.array(y0, copy=True), []
    for it in range(len(cfgs)):
        w = inp["b"] + B @ (sq * O.noise_rows(k, seed_w, ctr_w + it))
        (y,), ctr_s = expected_gibbs(op, [cfg.sampler], seed_s, ctr_s, y, b=w)
        y = y - G @ (B.T @ y)
        out.append(y.copy())
    return out, ctr_w + len(cfgs), ctr_s


def expected_samples(c, seed, ctr0, y0=None, guesszero=False, inner=None):
    """the NSAMPLES expected samples of a chain case and the PC's counter after them; inner = (seed, counter) of a woodbury
    PC's inner sampler"""
    y0 = inputs(c.op)["y0"] if y0 is None else y0
    kind = c.expect[0]
    if isinstance(kind, Gibbs):
        return expected_gibbs(c.op, c.expect, seed, ctr0, y0)
    if isinstance(kind, MG):
        return expected_mg(c.op, c.expect, seed, ctr0, y0, guesszero)
    if isinstance(kind, Chol):
        return expected_chol(c.op, c.expect, seed, ctr0)
    if isinstance(kind, Woodbury):
        out, cw, _ = expected_woodbury(c.op, c.expect, seed, ctr0, inner[0], inner[1], y0)
        return out, cw
    raise TypeError(kind)


def tolerance(c):
    """relative, the one the direct-handle test of the same operation uses: 1e-13 single-level sweep (test_gpu_grid.py,
    test_gpu_mcsor.py), 1e-11 V-cycle (test_gpu_mgmc.py) and Woodbury (test_gpu_pc_layer.py), 1e-12 cholsampler
    (test_gpu_mgmc.py); 1e-10 the V-cycle on a MATLRC operator (test_lrc.py::test_device_mgmc_lrc_matches_oracle)"""
    kind = c.expect[0]
    if isinstance(kind, Gibbs):
        return 1e-13
    if isinstance(kind, MG):
        return 1e-10 if inputs(c.op)["B"] is not None else 1e-11
    if isinstance(kind, Chol):
        return 1e-12
    return 1e-11
