"""The search forest over IntervalSet stores with formula units on the GPU (-m gpu): setformdfs_kernel (pcp_amd/csrc/pcp_setformdfs.hip,
pcp_dfs_forest_device_setform / _setform_bnb) against figures computed on the CPU — the oracle's own search and the restatements of
setform_forest_ref.py and test_bnb_forest_cpu.py, which test_setform_forest_cpu.py pins — never against the code under test."""
import ctypes as C
import re

import numpy as np
import pytest

from pcp_amd import model as M
from pcp_amd import search_forest as SF

import setform_cases as SC
import setform_forest_ref as R
from test_set_mode import random_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


def push(ctx, vs, cs, sw=1, hull=(0, 63)):
    M.push_model(ctx, cs, len(vs), sw)
    ctx.set_hull(*hull)


def counts(r):
    assert r["error"] == 0, r
    return r["nodes"], r["solutions"], r["failed"]


def check_plan(ctx, n_trees):
    """One wavefront per tree, four trees per 256-thread workgroup (these stores are a few hundred bytes each)."""
    pl = ctx.last_plan()
    assert pl["path"] == 3 and pl["set_mode"] == 1 and pl["block"] == 256 and pl["grid"] == -(-n_trees // 4) and 0 < pl["lds_bytes"] <= 80 * 1024, pl


@pytest.mark.parametrize("brancher,val", R.BRANCHERS)
def test_one_tree_is_the_reference_node_for_node(ctx, brancher, val):
    """The 4-task schedule, horizon 8: all solutions in one launch, in launches of 3 nodes (persist / resume: every unit live again at
    launch start), at a node limit of 20 (StopNode's last node), and the first solution."""
    vs, cs, _ = R.schedule(R.DUR4, 8, False)
    push(ctx, vs, cs)
    root = SC.hull_sets(vs, 1, 0)[None]
    want = R.schedule_counts(R.DUR4, 8, False, brancher, val)
    r = ctx.dfs_forest_setform(root, brancher=brancher, val=val)
    check_plan(ctx, 1)
    print("one tree", brancher, val, counts(r), want)
    assert counts(r) == want and r["finished_trees"] == 1 and r["launches"] == 1 and not r["stopped"]
    r3 = ctx.dfs_forest_setform(root, brancher=brancher, val=val, steps_per_launch=3)
    print("launches of 3", counts(r3), r3["launches"])
    assert counts(r3) == want and r3["finished_trees"] == 1 and r3["launches"] >= want[0] // 3
    for steps in (256, 3):
        rl = ctx.dfs_forest_setform(root, brancher=brancher, val=val, node_limit=20, steps_per_launch=steps)
        print("node limit 20", steps, counts(rl))
        assert counts(rl) == R.schedule_counts(R.DUR4, 8, False, brancher, val, 20) and rl["total_nodes"] == 20 and rl["stopped"]
    rs = ctx.dfs_forest_setform(root, brancher=brancher, val=val, stop_on_solution=True)
    assert rs["solutions"] == 1 and rs["stopped"] and rs["first_solution"] is not None and R.schedule_is_valid(rs["first_solution"])


@pytest.mark.parametrize("seed", [0, 4, 6, 7, 8, 9])
def test_random_formula_stores(ctx, seed):
    """12 variables, about 10 random units, from the hull, 2000 nodes at most: seeds 6 and 8 finish below the limit, 4, 7 and 9 reach it,
    seed 0 fails at the root (a one-node tree)."""
    vs, cs, _ = SC.random_case(seed)
    lb0, ub0 = vs.bounds()
    ss = SC.oracle_model(vs, cs).search_set(lb0, ub0, 1, 0, all_solutions=True, node_limit=2000)[0]
    want = (ss["num_nodes"], ss["num_solution"], ss["num_failed_node"])
    assert (want == (1, 0, 1)) == (seed == 0) and (want[0] == 2000) == (seed in (4, 7, 9))
    push(ctx, vs, cs, 1, (0, 6))
    r = ctx.dfs_forest_setform(SC.hull_sets(vs, 1, 0)[None], node_limit=2000)
    print("random store", seed, counts(r), want)
    assert counts(r) == want and (r["finished_trees"] == 1) == (want[0] < 2000)


def test_word_boundary(ctx):
    """set_words = 2 from -60: the domains 0..7 straddle words 0 and 1."""
    vs, cs, _ = R.schedule(R.DUR4, 8, False)
    push(ctx, vs, cs, 2, (-60, 67))
    root = SC.hull_sets(vs, 2, -60)[None]
    assert (root[0, :4, 0] >> np.uint64(60)).all() and (root[0, :4, 1] & np.uint64(1)).all()
    assert R.schedule_counts(R.DUR4, 8, False) == (61, 24, 7)
    for brancher, val in R.BRANCHERS:
        r = ctx.dfs_forest_setform(root, brancher=brancher, val=val, steps_per_launch=16)
        print("word boundary", brancher, val, counts(r))
        assert counts(r) == R.schedule_counts(R.DUR4, 8, False, brancher, val) and r["finished_trees"] == 1


def test_more_than_64_units_and_a_unit_of_more_than_64_nodes(ctx):
    """70 units: lanes take a second unit each inside the tree kernel (the oracle: a 5-node tree below the hull).  Distinct over 12
    variables next to an equivalence: a flat Conjunction of 67 tree nodes, walked by the member loop."""
    vs, cs, _ = SC.wide_case(500)
    assert len(cs) == 70
    lb0, ub0 = vs.bounds()
    ss = SC.oracle_model(vs, cs).search_set(lb0, ub0, 1, 0, all_solutions=True)[0]
    assert (ss["num_nodes"], ss["num_solution"], ss["num_failed_node"]) == (5, 0, 3)
    push(ctx, vs, cs, 1, (0, 6))
    assert counts(ctx.dfs_forest_setform(SC.hull_sets(vs, 1, 0)[None])) == (5, 0, 3)

    vs, cs = M.VStore(), M.CStore()
    xs = [vs.alloc((0, 13)) for _ in range(12)]
    b = vs.alloc((0, 1))
    cs.alloc(M.Distinct(xs))
    cs.alloc(M.equivalence(M.Boolean(b), M.XLessY(xs[0], xs[1])))
    lb0, ub0 = vs.bounds()
    om = SC.oracle_model(vs, cs)
    push(ctx, vs, cs, 1, (0, 13))
    # from the hull and from a node of random sets with holes: both reach the limit with solutions and failures behind them
    roots = [M.interval_bits(lb0, ub0, 1, 0), random_sets(611, lb0, ub0, 1, 1, 0, p_keep=0.5)[0]]
    seen = []
    for root in roots:
        ss = om.search_set(None, None, 1, 0, all_solutions=True, node_limit=600, root_bits=root)[0]
        want = (ss["num_nodes"], ss["num_solution"], ss["num_failed_node"])
        r = ctx.dfs_forest_setform(root[None], node_limit=600)
        print("Distinct(12) + equivalence", counts(r), want)
        assert counts(r) == want
        seen.append(want)
    assert all(w[0] == 600 and w[1] > 0 and w[2] > 0 for w in seen)


@pytest.mark.parametrize("brancher,val", R.BRANCHERS)
def test_forest(ctx, brancher, val):
    """The 4-task schedule, horizon 11: a breadth-first expansion to 8 open nodes, then 8 trees in launches of 4 nodes; expansion plus
    trees are one tree of the distributor.  With refill at least one finished tree takes over an open right branch."""
    vs, cs, _ = R.schedule(R.DUR4, 11, False)
    lb0, ub0 = vs.bounds()
    want = R.schedule_counts(R.DUR4, 11, False, brancher, val)
    if brancher == "split":
        assert want == (997, 490, 9)
    push(ctx, vs, cs)
    for rebalance in (True, False):
        r = SF.forest_search_set(ctx, lb0, ub0, 0, n_trees=8, steps_per_launch=4, brancher=brancher, val=val, formulas=True, rebalance=rebalance)
        print("forest", brancher, val, rebalance, r)
        assert r["trees"] >= 8 and r["seeded_nodes"] > 0
        check_plan(ctx, r["trees"])
        assert counts(r) == want and r["finished_trees"] == r["trees"]
        assert (r["splits"] >= 1) if rebalance else (r["splits"] == 0)


@pytest.mark.parametrize("durations,horizon", [(R.DUR4, 8), (R.DUR5, 16)])
@pytest.mark.parametrize("brancher,val", R.BRANCHERS)
def test_branch_and_bound_one_tree_is_the_reference_node_for_node(ctx, durations, horizon, brancher, val):
    vs, cs, m = R.schedule(durations, horizon, True)
    ref = R.schedule_bnb(durations, horizon, brancher, val)
    push(ctx, vs, cs)
    root = SC.hull_sets(vs, 1, 0)[None]
    for steps in (256, 3):
        r = ctx.dfs_forest_setform_bnb(root, (m, "min"), brancher=brancher, val=val, steps_per_launch=steps)
        print("bnb", durations, brancher, val, steps, counts(r), r["best"], (ref["nodes"], ref["solutions"], ref["failed"]), ref["best"])
        assert counts(r) == (ref["nodes"], ref["solutions"], ref["failed"]) and r["best"] == ref["best"] and r["finished_trees"] == 1
        row = r["best_solution"]
        assert row is not None and int(row[m]) == r["best"] and R.schedule_is_valid(row, durations, makespan=r["best"])
        assert np.array_equal(row, ref["row"])  # (one tree: the reference's own optimum row)


@pytest.mark.parametrize("n_trees", [1, 8, 64])
def test_branch_and_bound_forest(ctx, n_trees):
    """The 5-task schedule grown from one root: the optimum does not depend on the number of trees."""
    vs, cs, m = R.schedule(R.DUR5, 16, True)
    lb0, ub0 = vs.bounds()
    assert R.schedule_bnb(R.DUR5, 16)["best"] == 14
    push(ctx, vs, cs)
    for brancher, val in R.BRANCHERS:
        r = SF.forest_bnb_set(ctx, lb0, ub0, 0, (m, "min"), n_trees=n_trees, ramp_steps=2, steps_per_launch=64, brancher=brancher, val=val, formulas=True)
        print("bnb forest", n_trees, brancher, val, counts(r), r["best"], r["splits"], r["launches"])
        check_plan(ctx, n_trees)
        assert r["error"] == 0 and r["best"] == 14 and r["finished_trees"] == n_trees
        assert int(r["best_solution"][m]) == 14 and R.schedule_is_valid(r["best_solution"], R.DUR5, makespan=14)
        assert int(r["per_tree"][:, 0].sum()) == r["total_nodes"] == r["nodes"]


def test_refusals(ctx):
    import torch
    import pcp_amd.engine as E
    dev = torch.device("cuda", 0)

    def raw(obj=False, enumerate_=0, val=0, var=0, mode=0, null_best=False, V=None):
        """The C entry itself on a well-formed one-tree state."""
        V = V or ctx.n_vars
        sw = max(ctx.set_words, 1)
        t = {k: torch.zeros(s, dtype=d, device=dev) for k, (s, d) in
             {"bits": ((1, V, sw), torch.int64), "tree": ((1, 4), torch.int32), "levels": ((1, 64, 4), torch.int32), "trail": ((1, 64, 4), torch.int32),
              "counters": ((1, 4), torch.int64), "glob": ((4,), torch.int64), "best": ((1,), torch.int32), "tree_best": ((1,), torch.int32)}.items()}
        st = E.ForestState(1, 64, 64, 0, t["bits"].data_ptr(), t["tree"].data_ptr(), t["levels"].data_ptr(), t["trail"].data_ptr(), t["counters"].data_ptr(),
                           t["glob"].data_ptr(), t["glob"].data_ptr() + 8, None, None)
        if not obj:
            return ctx._L.pcp_dfs_forest_device_setform(ctx._h, C.byref(st), enumerate_, val, 4, 0, 0, None)
        o = E.ForestObjective(var, mode, None if null_best else t["best"].data_ptr(), t["tree_best"].data_ptr(), None)
        return ctx._L.pcp_dfs_forest_device_setform_bnb(ctx._h, C.byref(st), C.byref(o), enumerate_, val, 4, 0, None)

    # a set-mode store without formula units: the records forest searches it
    n = 6
    ctx.set_model(n, M.nqueens_props(n), set_words=1)
    ctx.set_hull(1, n)
    root = M.interval_bits(np.ones(n, np.int32), np.full(n, n, np.int32), 1, 1)[None]
    for call in (lambda: ctx.dfs_forest_setform(root), lambda: ctx.dfs_forest_setform_bnb(root, (0, "min"))):
        with pytest.raises(E.PcpError) as e:
            call()
        assert e.value.code == -5 and re.search(r"\bpcp_dfs_forest_device_set\b", str(e.value))
    assert ctx.dfs_forest_set(root)["solutions"] == 4
    # an interval-mode model
    ctx.set_model(n, M.nqueens_props(n))
    assert raw() == -1 and raw(obj=True) == -1
    # a formula store: the arguments
    vs, cs, m = R.schedule(R.DUR4, 8, True)
    push(ctx, vs, cs)
    assert raw(enumerate_=2) == -1 and raw(enumerate_=1, val=2) == -1 and raw(val=2) == -1
    assert raw(obj=True, enumerate_=2) == -1 and raw(obj=True, val=2) == -1
    assert raw(obj=True, var=len(vs)) == -1 and raw(obj=True, mode=2) == -1 and raw(obj=True, null_best=True) == -1
    root = SC.hull_sets(vs, 1, 0)[None]
    with pytest.raises(E.PcpError) as e:  # the records forest keeps refusing it, and says where to go
        ctx.dfs_forest_set(root)
    assert e.value.code == -5 and "formula" in str(e.value) and "pcp_dfs_forest_device_setform" in str(e.value)
    for brancher in ("split", "enumerate"):
        with pytest.raises(E.PcpError) as e:
            ctx.dfs_forest_set_bnb(root, (m, "min"), brancher=brancher)
        assert e.value.code == -5 and "formula" in str(e.value)
    assert ctx.dfs_forest_setform_bnb(root, (m, "min"))["best"] == 8  # ... and the store is intact
