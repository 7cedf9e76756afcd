"""Enumerate in the formula-store forest (pcp_dfs_forest_device_form_enum), without a GPU: the header declares and the library exports the
entry and the Python drivers exist; FormTreeSim (form_enum_forest_cases.py) — the restatement of one tree's rows, row words and exclusion
path that test_form_enum_forest_gpu.py compares the device with at every launch seam — visits exactly the nodes of the host specification
(search.dfs_enumerate at batch 1 over the oracle-backed stand-in, test_form_excl_cpu.reference_bnb_enum under an objective) with the same
lists, counts and incumbents; and the conditions that keep the GPU tests from being vacuous."""
import inspect
import os
import re

import numpy as np
import pytest

import form_enum_forest_cases as EC
import form_excl_cases as X
from pcp_amd import search as S
from test_form_excl_cpu import FormExclOracleCtx, _objective, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pcp_dfs_forest_device_form_enum"


def test_the_header_declares_and_the_library_exports_the_entry():
    """Fails without the feature: neither the header nor the ctypes and Rust lists name the entry, and the two drivers do not exist."""
    import pcp_amd.engine as E
    import pcp_amd.search_forest as SF
    import test_abi
    with open(os.path.join(ROOT, "include", "pcp_hip.h")) as f:
        header = f.read()
    m = re.search(r"\bint32_t\s+" + NAME + r"\s*\(([^)]*)\)", header)
    small = re.search(r"\bint32_t\s+pcp_dfs_forest_device_small_enum\s*\(([^)]*)\)", header)
    assert m and small and m.group(1).split() == small.group(1).split()  # the signature of the small-store entry
    assert NAME in E.ABI_SYMBOLS and hasattr(test_abi._built(), NAME)
    with open(os.path.join(ROOT, "pcp_amd", "engine.py")) as f:
        assert f"L.{NAME}.argtypes" in f.read()
    with open(os.path.join(ROOT, "integration", "pcp-hip-sys", "src", "lib.rs")) as f:
        assert "pub fn " + NAME in f.read()
    p = inspect.signature(E.Context.dfs_forest_enum).parameters
    want = dict(val="middle", objective=None, best0=None, root_excl=None, path_capacity=64, max_path=1 << 20, collect_solutions=False, sink_capacity=4096)
    assert {k: p[k].default for k in want} == want
    assert list(p)[:3] == ["self", "root_lb", "root_ub"] and {"steps_per_launch", "capacity", "max_capacity", "rebalance", "info", "node_limit_per_tree"} <= set(p)
    p = inspect.signature(SF.forest_enumerate).parameters
    want = dict(val="middle", objective=None, collect_solutions=False, sink_capacity=4096, info=None)
    assert {k: p[k].default for k in want} == want and list(p)[:3] == ["ctx", "lb0", "ub0"] and {"n_trees", "steps_per_launch"} <= set(p)


def test_the_new_calls_refuse_before_anything_runs():
    import pcp_amd.engine as E
    from pcp_amd.search_forest import forest_enumerate
    for kw in (dict(dist=object()), dict(val="largest"), dict(collect_solutions=True, objective=(0, "min"))):
        with pytest.raises(ValueError):
            E.Context.dfs_forest_enum(None, None, None, **kw)
        with pytest.raises(ValueError):
            forest_enumerate(None, None, None, **kw)


_SPEC = {}


def spec(name, val):
    """search.dfs_enumerate at batch 1 over the stand-in, every solution, once per case: (SearchStats, records).  The complete tree, or its
    first form_enum_forest_cases.WALK_LIMIT nodes under StopNode."""
    if (name, val) not in _SPEC:
        key = "search:" + name
        lb0, ub0 = EC.root_of(key)
        rec = []
        _SPEC[(name, val)] = (S.dfs_enumerate(FormExclOracleCtx(key), lb0, ub0, all_solutions=True, batch=1, val=val, record=rec,
                                                 node_limit=EC.WALK_LIMIT.get(name, 0)), rec)
    return _SPEC[(name, val)]


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("name", EC.SEARCH_NAMES)
def test_the_simulator_visits_the_specifications_nodes_with_the_same_lists(name, val):
    st, rec = spec(name, val)
    sim = EC.FormTreeSim("search:" + name, val, node_limit=EC.WALK_LIMIT.get(name, 0))
    seen = []

    def on_node(s):
        L, U, lst, status, lb, ub = s.last
        r = rec[len(seen)]
        assert np.array_equal(L, r[0]) and np.array_equal(U, r[1]) and status == r[3], len(seen)
        assert EC.inside(lst, L, U) == EC.inside(r[2], L, U) == {(int(x), int(v)) for x, v in r[2]}, len(seen)
        if status:
            assert np.array_equal(lb, r[4]) and np.array_equal(ub, r[5]), len(seen)
        assert all(a <= b for a, b in zip(s.row_base, s.row_base[1:]))  # row_base does not decrease with r
        seen.append(1)

    got = sim.run(on_node)
    print(name, val, got, "max_path", sim.max_path, "rechosen", sim.rechosen)
    assert got == EC.counts(st) and len(seen) == len(rec)
    assert 0 < sim.nodes <= X.TREE_CEILING and sim.nodes == (EC.WALK_LIMIT.get(name) or sim.nodes)
    assert (sim.sp > 0) == (name in EC.WALK_LIMIT)  # a walk that ends at its limit leaves open nodes; every other tree is complete
    if val == "min":
        assert sim.max_path == 0 and sim.rechosen == 0
    else:
        assert sim.max_path >= 1 and sim.rechosen > 0
    if name == "A4":  # the boxes hold every schedule once
        pts, total = X.covered(4, sim.boxes)
        assert pts == set(X.all_schedules("A4")) and total == len(pts)


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("name", EC.SEARCH_NAMES)
def test_the_simulator_under_branch_and_bound(name, val):
    var, mode = _objective(name)
    ref = reference(name, val)
    sim = EC.FormTreeSim("search:" + name, val, objective=(var, mode))
    got = sim.run()
    print(name, val, mode, got, sim.incumbents)
    assert got == (ref["nodes"], ref["solutions"], ref["failed"]) and sim.nodes <= X.TREE_CEILING
    assert sim.incumbents == ref["incumbents"] and sim.best == ref["best"] and np.array_equal(sim.best_row, ref["row"])
    if val == "min":
        assert sim.max_path == 0


def test_a_value_excluded_already_is_not_chosen_again():
    """rechosen > 0: every named model reaches it by itself under MiddleVal (asserted above, and under branch and bound here) — A4's tree
    first at its node 16, where MiddleVal's value of the variable FirstSmallestVar picks is in the node's list already and the lower
    neighbour is taken.  No constructed root is needed."""
    sim = EC.FormTreeSim("search:A4", "middle")
    while not sim.rechosen:
        sim.step()
    assert sim.nodes == 16 and sim.last[3] == 2
    L, U, lst, _, lb, ub = sim.last
    x = int(S.first_smallest_var(lb[None], ub[None])[0])
    m = int(S.middle_val(lb[x:x + 1], ub[x:x + 1])[0])
    left = sim.top()
    assert (x, m) in lst and left[0][x] == left[1][x] == m - 1 and (x, m - 1) not in lst
    for name in EC.SEARCH_NAMES:
        bnb = EC.FormTreeSim("search:" + name, "middle", objective=_objective(name))
        bnb.run()
        assert bnb.rechosen > 0 and bnb.max_path >= 1, name


def test_the_sweep_roots_are_what_they_are_there_for():
    roots = EC.sweep_roots()
    sizes = [len(e) for _, _, e in roots]
    assert sizes[:4] == list(EC.SWEEP_SIZES) and X.CHAIN in sizes
    for (lb0, ub0, ex), c in zip(roots, EC.SWEEP_SIZES):
        st, lb, ub = EC.judge("wide", lb0, ub0, ex)
        base = EC.judge("wide", lb0, ub0, [])
        assert st == 2 and lb[1] >= 1 and ub[2] <= 99 and base[1][1] == 0 and base[2][2] == 100  # the entries at the bounds moved them
        assert any(not (lb0[x] <= v <= ub0[x]) for x, v in ex) and any(lb[x] < v < ub[x] for x, v in ex)
