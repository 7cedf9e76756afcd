"""The forest over small Interval stores of plain propagators (pcp_dfs_forest_device_small, _small_bnb), without a GPU: the header
declares and the library exports the entries, and the figures test_small_forest_gpu.py compares the device with — the oracle's DFS and the
host specification of branch and bound (pcp_amd.search.dfs with an objective, batch = 1, over the oracle) on the models of
small_forest_cases.py — are pinned as literals."""
import inspect
import os
import re

import pytest

import form_forest_cases as FC
import small_forest_cases as C
from pcp_amd import search as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (nodes, solutions, failed) of the oracle's search, all solutions, from the store's root; the stores under C.NODE_LIMIT
GOLOMB_TREE = {5: (1391, 607, 89), 6: (17695, 6606, 2242)}
GOLOMB_FIRST = {5: ((15, 1, 0), [0, 1, 3, 7, 12])}
QUEENS8 = (779, 92, 298)
STORE_TREE = {
    "two-distincts": (2000, 992, 0), "wide-distinct": (2000, 971, 1), "distinct64": (2000, 872, 0), "many-units": (1763, 882, 0),
    "slots128": (2000, 996, 0), "recs2048": (2000, 962, 0), "mixed-7100": (187, 85, 9), "mixed-7101": (2000, 486, 506),
    "mixed-7102": (2000, 725, 265), "mixed-7103": (2000, 991, 2), "mixed-7104": (2000, 847, 152), "mixed-7105": (2000, 420, 573),
}
# the host specification of branch and bound: (best, (nodes, solutions, failed))
GOLOMB_BNB = {(5, "min"): (11, (41, 2, 19)), (5, "max"): (20, (37, 7, 12)), (6, "min"): (17, (143, 3, 69)), (6, "max"): (30, (49, 8, 17))}


def test_the_header_declares_and_the_library_exports_the_two_entries():
    """Fails without the feature: neither the header nor ABI_SYMBOLS names the entries."""
    import pcp_amd.engine as E
    import pcp_amd.search_forest as SF
    import test_abi
    with open(os.path.join(ROOT, "include", "pcp_hip.h")) as f:
        header = f.read()
    L = test_abi._built()
    for name in ("pcp_dfs_forest_device_small", "pcp_dfs_forest_device_small_bnb"):
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", header), name
        assert name in E.ABI_SYMBOLS and hasattr(L, name)
    assert "no forest: pcp_dfs_device" in header and re.search(r"small stores, Interval\s+pcp_dfs_forest_device_small, _small_bnb", header)
    for fn in (E.Context.dfs_forest, E.Context.dfs_forest_bnb, SF.forest_search, SF.forest_bnb):
        assert inspect.signature(fn).parameters["small"].default is False
    assert inspect.signature(SF.forest_bnb).parameters["formulas"].default is True


def test_small_and_formulas_together_are_refused_before_anything_runs():
    from pcp_amd.search_forest import forest_search
    import pcp_amd.engine as E
    with pytest.raises(ValueError):
        forest_search(None, None, None, formulas=True, small=True)
    with pytest.raises(ValueError):
        E.Context.dfs_forest(None, None, None, formulas=True, small=True)


@pytest.mark.parametrize("m", [5, 6])
def test_the_oracles_complete_tree_of_golomb(m):
    """m = 5 is the model of the one-step-per-launch tests: 1391 nodes, under the 2500 such a test may take."""
    vs, cs, var = C.golomb(m)
    assert var == m - 1 and len(vs) == m + m * (m - 1) // 2 and len(cs) == 2 + m + m * (m - 1) // 2
    om = FC.oracle_model(vs, cs)
    lb0, ub0 = vs.bounds()
    assert FC.counts(om.search(lb0, ub0, all_solutions=True)[0]) == GOLOMB_TREE[m]
    if m in GOLOMB_FIRST:
        ss1, _, _, sol1 = om.search(lb0, ub0, all_solutions=False)
        assert FC.counts(ss1) == GOLOMB_FIRST[m][0] and sol1[:m].tolist() == GOLOMB_FIRST[m][1] and C.is_ruler(sol1, m)


@pytest.mark.parametrize("m,mode", sorted(GOLOMB_BNB))
def test_the_host_specification_of_branch_and_bound_on_golomb(m, mode):
    vs, cs, var = C.golomb(m)
    lb0, ub0 = vs.bounds()
    st = S.dfs(FC.FormulaOracleCtx(vs, cs), lb0, ub0, objective=(var, mode), batch=1)
    assert (st.best, FC.counts(st)) == GOLOMB_BNB[(m, mode)]
    assert int(st.best_solution[var]) == st.best and C.is_ruler(st.best_solution, m)
    if mode == "min":
        assert st.best == C.OPTIMUM[m] == {5: 11, 6: 17}[m]


def test_the_shifted_ruler_descends_for_ever():
    """Marks from -3: MiddleVal of (-1, 0) is 0 — (lb + ub) / 2 truncates toward zero — so the left child is its parent again."""
    vs, cs = C.golomb_shifted(5, -3)
    lb0, ub0 = vs.bounds()
    assert lb0[0] == -3 and ub0[0] == C.LENGTH[5] - 3
    assert FC.counts(FC.oracle_model(vs, cs).search(lb0, ub0, all_solutions=True, node_limit=200)[0]) == (200, 0, 0)


def test_queens8():
    vs, cs = C.queens8()
    assert FC.counts(FC.oracle_model(vs, cs).search(*vs.bounds(), all_solutions=True)[0]) == QUEENS8 and QUEENS8[1] == 92


@pytest.mark.parametrize("name", sorted(C.STORES))
def test_the_oracles_tree_of_the_stores(name):
    vs, cs = C.store(name)
    om = FC.oracle_model(vs, cs)
    assert FC.counts(om.search(*vs.bounds(), all_solutions=True, node_limit=C.NODE_LIMIT)[0]) == STORE_TREE[name]


def test_the_stores_have_the_shapes_they_are_named_for():
    import small_cases as SC
    from pcp_amd import model as M
    shape = lambda f: (lambda vs, cs: (len(vs), len(cs.props), SC.slot_count(cs.props, len(vs))))(*f())
    assert shape(C.slots128)[2] == 128 and shape(C.slots128)[1] <= 2048 and shape(C.slots128)[0] > 64
    assert shape(C.recs2048)[1] == 2048 and shape(C.recs2048)[2] <= 128
    assert shape(C.slots129)[2] == 129 and shape(C.slots129)[1] <= 2048
    assert shape(C.recs2049)[1] == 2049 and shape(C.recs2049)[2] <= 128
    assert len(C.many_units()[1]) > 64
    # the Distinct units the engine filters as groups: two in one store; 64 variables in one; a root hull beyond the 128-value mask
    ad = lambda name: SC.alldiff_units(C.store(name)[1].lower(len(C.store(name)[0])), len(C.store(name)[0]))[0]
    assert [len(v) for _, v in ad("two-distincts")] == [6, 5]
    assert [len(v) for _, v in ad("distinct64")] == [64]
    vs, cs = C.store("wide-distinct")
    (_, unit), = ad("wide-distinct")
    lb0, ub0 = vs.bounds()
    assert int(ub0[unit].max()) - int(lb0[unit].min()) >= 128
    for s in C.MIXED_SEEDS:  # ternary kinds, a Constant operand, a Sum view, an XEqYMulZ, a Distinct
        units = C.store(f"mixed-{s}")[1].units
        kinds = {u.kind for u in units if isinstance(u, M.Elementary)}
        assert kinds & {M.LT3, M.GT3, M.EQ3} and M.MUL3 in kinds and any(isinstance(u, M.Conjunction) for u in units)
        ops = [o for u in units if isinstance(u, M.Elementary) for o in u.ops]
        assert any(isinstance(o, M.Constant) for o in ops)
        assert any(isinstance(o, M.Sum) or isinstance(getattr(o, "x", None), M.Sum) or "Sum(" in repr(o) for o in ops)
