#!/usr/bin/env python3
"""Record MGMC.algorithmic_bytes() -- (total, per_level) of pmg_mgmc_get_algorithmic_bytes -- for a fixed list of small
hierarchies into tests/golden/cycle_bytes.json.  tests/test_gpu_cycle_bytes.py imports the list from here and compares
with exact equality: every term of the model is a product of integers held in doubles far below 2^53.

usage: record_cycle_bytes.py [out.json]     (needs a GPU: the byte model reads a hierarchy that has been set up)"""
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "cycle_bytes.json")

# one set-up per group; pmg_mgmc_set_correction_form and (on one device) pmg_mgmc_set_fused_transfers are flipped on it
# afterwards, as the library allows
DMDA_GROUPS = [(n, levels, coarse, sweep, k) for (n, levels) in ((33, 3), (65, 4)) for coarse in ("cholsampler", "gibbs") for sweep in ("forward", "symmetric") for k in (0, 3)]
TOGGLES = list(itertools.product(("inplace", "literal"), ("fused", "unfused")))
OTHER_GROUPS = ["dmda33_3_scaled_omega1.2", "aij_lshape_refine2"]


def group_name(g):
    return g if isinstance(g, str) else "dmda%d_%d_%s_%s_k%d" % g


GROUPS = DMDA_GROUPS + OTHER_GROUPS


def observation_mats(n, k):
    """the k ball observations of tools/cyclebench.py's low-rank line"""
    from parmgmc_amd import make_observation_mats

    centres = [(0.25, 0.25, 0.25), (0.75, 0.75, 0.75), (0.25, 0.75, 0.5)]
    return make_observation_mats(n, n, n, np.asarray(centres[:k]).ravel(), [0.1, 0.15, 0.1][:k], np.resize([1.0, -1.0], k), 1e-4)


def lshape_hierarchy(refine):
    """the caller-supplied AIJ hierarchy of tools/cyclebench.py's mgmc_aij line, at a smaller refinement"""
    from parmgmc_amd.unstructured import assemble_p1, build_hierarchy, read_gmsh41_triangles, refine_uniform

    xy, tris = read_gmsh41_triangles(os.path.join(ROOT, "tests", "golden", "lshape.msh"))
    for _ in range(refine):
        xy, tris = refine_uniform(xy, tris)
    return build_hierarchy(assemble_p1(xy, tris, 1.0), coarse_max=2000)


def setup_group(g):
    from parmgmc_amd import COLORING_ITERATED, MGMC, SOR_FORWARD_SWEEP, SOR_SYMMETRIC_SWEEP

    if g == "aij_lshape_refine2":
        mg = MGMC.from_hierarchy(*lshape_hierarchy(2))
        mg.set_coloring(COLORING_ITERATED)
        mg.set_smoother(True, 1.0, 1, 1)
        return mg.setup()
    if g == "dmda33_3_scaled_omega1.2":
        mg = MGMC(33, 33, 33, 10.0, 3)
        mg.set_smoother(True, 1.2, SOR_FORWARD_SWEEP, 1)
        return mg.setup()
    n, levels, coarse, sweep, k = g
    mg = MGMC(n, n, n, 10.0, levels)
    mg.set_smoother(False, 1.0, {"forward": SOR_FORWARD_SWEEP, "symmetric": SOR_SYMMETRIC_SWEEP}[sweep], 1)
    mg.set_coarse(coarse, 1)
    if k:
        B, S, _ = observation_mats(n, k)
        mg.set_lowrank(B, S)
    return mg.setup()


def group_bytes(g):
    """{configuration name: [total, [per level]]} of one group"""
    mg = setup_group(g)
    out = {}
    for form, transfers in TOGGLES:
        mg.set_correction_form(form == "literal")
        mg.set_fused_transfers(transfers == "fused")
        total, per = mg.algorithmic_bytes()
        out["%s_%s_%s" % (group_name(g), form, transfers)] = [float(total), [float(x) for x in per]]
    mg.destroy()
    return out


def main():
    out = {}
    for g in GROUPS:
        out.update(group_bytes(g))
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d configurations -> %s" % (len(out), path))


if __name__ == "__main__":
    main()
