"""The catalogue of tests/handle_steps.py is complete and its orders are distinct (no GPU): an entry point added to
parmgmc_amd/wrappers.py has to be added to the catalogue, or to its exclusion table with a reason."""
import inspect
import re

import pytest

import handle_steps as H

DEVICE_METHOD = re.compile(r"^(sample|apply|run|residual|sweep_|level_|to_|from_)|^(update|reset)$")
# methods the patterns catch that take no device vector
NO_DEVICE_VECTOR = {
    "MGMC.from_hierarchy": "constructor", "ChainCov.from_chol": "constructor", "ChainCov.from_csr": "constructor", "ChainCov.from_dense": "constructor",
    "MGMC.level_dims": "host query", "MGMC.level_matrix": "host query", "MGMC.level_layout": "host query", "MGMC.level_stencil": "host query",
    "MGMC.level_lowrank_factors": "host query", "MGMC.level_lowrank_sizes": "host query",
}


def wrapper_methods():
    from parmgmc_amd import wrappers

    out = []
    for cname, cls in inspect.getmembers(wrappers, inspect.isclass):
        if cls.__module__ != wrappers.__name__:
            continue
        out += [f"{cname}.{m}" for m, f in vars(cls).items() if DEVICE_METHOD.search(m) and (inspect.isfunction(f) or isinstance(f, classmethod))]
    return sorted(out)


@pytest.mark.parametrize("kind", list(H.KINDS))
def test_step_names_are_unique_per_handle_kind(kind):
    cases, _, _, steps, failing = H.KINDS[kind]
    assert cases and len(set(cases)) == len(cases)
    for case in cases:
        names = [s.name for s in steps(case)]
        assert names and len(set(names)) == len(names), (kind, case, names)
        for s in steps(case):
            assert s.const and callable(s.fn), (kind, case, s.name)


def test_every_wrapper_method_that_takes_device_vectors_is_in_a_step():
    methods = wrapper_methods()
    assert len(methods) > 30 and "MGMC.level_residual_restrict" in methods and "ChainStats.update" in methods, methods
    used = {c for kind, (cases, _, _, steps, _) in H.KINDS.items() for case in cases for s in steps(case) for c in s.calls}
    for name, reason in {**H.EXCLUDED, **NO_DEVICE_VECTOR}.items():
        assert reason and name not in used, name
    missing = [m for m in methods if m not in used and m not in H.EXCLUDED and m not in NO_DEVICE_VECTOR]
    assert not missing, f"in no step of tests/handle_steps.py and not in its exclusion table: {missing}"
    from parmgmc_amd import pc, wrappers

    stale = [c for c in used if not hasattr(getattr(pc if c.startswith("PC.") else wrappers, c.split(".")[0]), c.split(".")[1])]
    assert not stale, f"steps name methods that do not exist: {stale}"


@pytest.mark.parametrize("kind", list(H.KINDS))
def test_the_five_orders_differ(kind):
    cases, _, _, steps, _ = H.KINDS[kind]
    for case in cases:
        names = [s.name for s in steps(case)]
        orders = H.orders(names)
        assert list(orders) == ["listed", "reversed"] + [f"perm{s}" for s in H.PERMUTATION_SEEDS] and len(H.PERMUTATION_SEEDS) == 3
        for o in orders.values():
            assert sorted(o) == sorted(names)
        assert len(names) >= 4 and len({tuple(o) for o in orders.values()}) == 5, (kind, case, orders)
