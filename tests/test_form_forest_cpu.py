"""The forest over Interval stores with formula units (pcp_dfs_forest_device_form, _form_bnb), without a GPU: the library exports the
entries, and the figures test_form_forest_gpu.py compares the device with — the oracle's DFS and the host specification of branch and
bound (pcp_amd.search.dfs with an objective) on the schedule models of form_forest_cases.py — are pinned."""
import inspect

import numpy as np
import pytest

import form_forest_cases as FC
from pcp_amd import search as S


def test_the_library_exports_the_forest_entries_for_interval_formula_stores():
    import pcp_amd.engine as E
    import pcp_amd.search_forest as SF
    import test_abi
    L = test_abi._built()
    for name in ("pcp_dfs_forest_device_form", "pcp_dfs_forest_device_form_bnb"):
        assert name in E.ABI_SYMBOLS and hasattr(L, name)
    assert inspect.signature(E.Context.dfs_forest).parameters["formulas"].default is False
    assert callable(E.Context.dfs_forest_bnb)
    assert inspect.signature(SF.forest_search).parameters["formulas"].default is False
    assert inspect.signature(SF.forest_bnb).parameters["formulas"].default is True


def test_the_model_shapes():
    for name, (n_vars, n_units) in {"A4": (29, 28), "C4mk": (30, 32), "D5mk": (47, 50), "B5": (46, None), "six": (67, 66)}.items():
        vs, cs, _ = FC.schedule(name)
        assert len(vs) == n_vars and (n_units is None or len(cs) == n_units)


def test_the_oracles_complete_tree_of_a4():
    vs, cs, _ = FC.schedule("A4")
    om = FC.oracle_model(vs, cs)
    lb0, ub0 = vs.bounds()
    assert FC.counts(om.search(lb0, ub0, all_solutions=True)[0]) == (2025, 375, 638)
    ss1, _, _, sol1 = om.search(lb0, ub0, all_solutions=False)
    assert FC.counts(ss1) == (32, 1, ss1["num_failed_node"]) and FC.is_schedule("A4", sol1)


@pytest.mark.parametrize("name,mode,best,nodes", [("C4mk", "min", 5, 249), ("C4mk", "max", 12, 41), ("D5mk", "min", 7, 2235), ("D5mk", "max", 14, 59)])
def test_the_host_specification_of_branch_and_bound(name, mode, best, nodes):
    vs, cs, mk = FC.schedule(name)
    lb0, ub0 = vs.bounds()
    st = S.dfs(FC.FormulaOracleCtx(vs, cs), lb0, ub0, objective=(mk, mode), batch=1)
    assert (st.best, st.num_nodes) == (best, nodes)
    assert int(st.best_solution[mk]) == best and FC.is_schedule(name, st.best_solution)
    if (name, mode) == ("C4mk", "min"):
        assert (st.num_solution, st.num_failed_node, st.incumbents) == (4, 121, [8, 7, 6, 5])


def test_the_six_task_store_passes_one_wavefront():
    """Slots and units both pass 64: every lane-strided loop of the kernel takes a second trip."""
    vs, cs, _ = FC.schedule("six")
    assert len(vs) > 64 and len(cs) > 64
    ss = FC.oracle_model(vs, cs).search(*vs.bounds(), all_solutions=True, node_limit=3000)[0]
    assert ss["num_nodes"] == 3000 and ss["num_solution"] > 0 and ss["num_failed_node"] > 0
