"""Enumerate in the small-store forest (pcp_dfs_forest_device_small_enum), without a GPU: the header declares and the library exports the
entry, the figures test_small_enum_forest_gpu.py compares the device with — the complete Enumerate trees of the host specification
(pcp_amd.search.dfs_enumerate, batch = 1, over the oracle-backed stand-in context) on the models of small_forest_cases.py — are pinned as
literals and checked against a fresh search, and TreeSim (small_enum_forest_cases.py), the restatement of one tree's rows, row words and
exclusion path, visits the specification's nodes in order with the same lists."""
import inspect
import os
import re

import numpy as np
import pytest

import small_enum_forest_cases as EC
import small_forest_cases as C
from pcp_amd import search as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (nodes, solutions, failed) of the complete Enumerate tree from the store's root, per value selector
ENUM_TREE = {
    ("golomb5", "middle"): (2019, 607, 403), ("golomb5", "min"): (1469, 607, 128),
    ("golomb6", "middle"): (33645, 6606, 10217), ("golomb6", "min"): (19147, 6606, 2968),
    ("queens8", "middle"): (1333, 92, 575), ("queens8", "min"): (779, 92, 298),
    ("golomb5-3", "min"): (1469, 607, 128),
}
# branch and bound under Enumerate: (best, (nodes, solutions, failed))
ENUM_BNB = {
    ("golomb5", "middle", "min"): (11, (73, 7, 30)), ("golomb5", "middle", "max"): (20, (15, 1, 7)),
    ("golomb5", "min", "min"): (11, (27, 2, 12)), ("golomb5", "min", "max"): (20, (19, 7, 3)),
    ("golomb6", "middle", "min"): (17, (389, 13, 182)), ("golomb6", "middle", "max"): (30, (23, 1, 11)),
    ("golomb6", "min", "min"): (17, (121, 3, 58)), ("golomb6", "min", "max"): (30, (23, 8, 4)),
}


def test_the_header_declares_and_the_library_exports_the_entry():
    """Fails without the feature: neither the header nor the ctypes and Rust lists name the entry."""
    import pcp_amd.engine as E
    import pcp_amd.search_forest as SF
    import test_abi
    with open(os.path.join(ROOT, "include", "pcp_hip.h")) as f:
        header = f.read()
    name = "pcp_dfs_forest_device_small_enum"
    assert re.search(r"\bint32_t\s+" + name + r"\s*\(", header)
    struct = re.search(r"typedef struct \{([^}]*)\} pcp_forest_excl;", header)
    assert struct and [w for w in re.findall(r"(\w+);", struct.group(1))] == ["path", "row_base", "row_excl", "path_capacity", "val"]
    assert name in E.ABI_SYMBOLS and hasattr(test_abi._built(), name)
    assert [f for f, _ in E.ForestExcl._fields_] == ["path", "row_base", "row_excl", "path_capacity", "val"]
    with open(os.path.join(ROOT, "integration", "pcp-hip-sys", "src", "lib.rs")) as f:
        rust = f.read()
    assert "pub fn " + name in rust and "pub struct pcp_forest_excl" in rust
    for fn in (E.Context.dfs_forest, E.Context.dfs_forest_bnb, SF.forest_search, SF.forest_bnb, SF.seed_roots_interval):
        p = inspect.signature(fn).parameters
        assert p["brancher"].default == "split" and p["val"].default == "middle"
    for fn in (E.Context.dfs_forest, E.Context.dfs_forest_bnb):
        assert inspect.signature(fn).parameters["root_excl"].default is None


def test_refused_combinations_are_raised_before_anything_runs():
    import pcp_amd.engine as E
    from pcp_amd.search_forest import forest_bnb, forest_search
    dist = object()
    for kw in (dict(small=True, dist=dist), dict(formulas=True), dict(), dict(small=True, val="largest")):
        with pytest.raises(ValueError):
            forest_search(None, None, None, brancher="enumerate", **kw)
        with pytest.raises(ValueError):
            E.Context.dfs_forest(None, None, None, brancher="enumerate", **kw)
    for kw in (dict(small=True, dist=dist), dict(), dict(small=True, val="largest")):
        with pytest.raises(ValueError):
            E.Context.dfs_forest_bnb(None, None, None, (0, "min"), brancher="enumerate", **kw)
    for kw in (dict(formulas=True), dict(small=True, val="largest")):
        with pytest.raises(ValueError):
            forest_bnb(None, None, None, (0, "min"), brancher="enumerate", **kw)
    with pytest.raises(ValueError):
        E.Context.dfs_forest(None, None, None, small=True, brancher="binary")
    with pytest.raises(ValueError):
        E.Context.dfs_forest(None, None, None, small=True, root_excl=[])  # lists need Enumerate


_SPEC = {}


def spec(name, val, objective=None):
    """The host specification's search, once per case: (SearchStats, records)."""
    key = (name, val, objective)
    if key not in _SPEC:
        V, props, lb0, ub0, _ = EC.model(name)
        rec = []
        _SPEC[key] = (S.dfs_enumerate(EC.stand_in(name), lb0, ub0, all_solutions=True, batch=1, val=val, record=rec, objective=objective), rec)
    return _SPEC[key]


@pytest.mark.parametrize("name,val", sorted(ENUM_TREE))
def test_the_complete_enumerate_trees(name, val):
    st, _ = spec(name, val)
    assert EC.counts(st) == ENUM_TREE[(name, val)]
    if name == "queens8":
        assert st.num_solution == 92
    if name.startswith("golomb"):
        m = int(name[6])
        assert all(C.is_ruler(s, m) for s in st.solutions[:50])


@pytest.mark.parametrize("name,val,mode", sorted(ENUM_BNB))
def test_the_host_specification_of_branch_and_bound_under_enumerate(name, val, mode):
    var = EC.model(name)[4]
    st, _ = spec(name, val, (var, mode))
    assert (st.best, EC.counts(st)) == ENUM_BNB[(name, val, mode)]
    m = int(name[6])
    assert int(st.best_solution[var]) == st.best and C.is_ruler(st.best_solution, m)
    if mode == "min":
        assert st.best == C.OPTIMUM[m]


@pytest.mark.parametrize("name,val", [("golomb5", "middle"), ("golomb5", "min"), ("golomb6", "middle"), ("golomb6", "min")])
def test_the_simulator_visits_the_specifications_nodes_with_the_same_lists(name, val):
    """One path and two words per row give, at every node, the list the specification's filtered CSR lists give: compared inside the
    domain, as sets.  MinVal never grows the path; MiddleVal on Golomb 6 re-chooses a value at least once."""
    st, rec = spec(name, val)
    sim = EC.TreeSim(name, val)
    seen = []

    def on_node(s):
        L, U, lst, status = s.last
        r = rec[len(seen)]
        assert np.array_equal(L, r[0]) and np.array_equal(U, r[1]) and status == r[3], len(seen)
        assert EC.inside(lst, L, U) == EC.inside(r[2], L, U) == {(int(x), int(v)) for x, v in r[2]}, len(seen)
        assert all(a <= b for a, b in zip(s.row_base, s.row_base[1:]))  # row_base does not decrease with r
        seen.append(1)

    assert sim.run(on_node) == EC.counts(st) == ENUM_TREE[(name, val)] and len(seen) == len(rec)
    if val == "min":
        assert sim.max_path == 0 and sim.rechosen == 0
    else:
        assert sim.max_path > 0
        if name == "golomb6":
            assert sim.rechosen > 0


@pytest.mark.parametrize("mode", ["min", "max"])
def test_the_simulator_under_branch_and_bound(mode):
    var = EC.model("golomb5")[4]
    st, _ = spec("golomb5", "middle", (var, mode))
    sim = EC.TreeSim("golomb5", "middle", objective=(var, mode))
    assert sim.run() == EC.counts(st) and sim.best == st.best
