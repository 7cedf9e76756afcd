"""The search forest over Interval stores with formula units on the device (pcp_dfs_forest_device_form, _form_bnb; pcp_formdfs.hip):
one tree against the oracle and against pcp_dfs_device node for node, expansion plus forest against the oracle's complete tree, refill and
growth, edge roots, branch and bound against the host specification, and the contract.  The models are the Cumulative schedules of
form_forest_cases.py; test_form_forest_cpu.py pins the figures the oracle and the host specification give on them."""
import numpy as np
import pytest

import form_forest_cases as FC
from pcp_amd import model as M
from pcp_amd import search as S
from test_reified import random_formula_store

pytestmark = pytest.mark.gpu

BOUND_MAX = (1 << 29) - 1


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


_cache = {}


def case(ctx, name, shift=0):
    """Push the model and return (vs, oracle model, lb0, ub0, makespan variable); the oracle's figures are computed once per model."""
    vs, cs, mk = FC.schedule(name, shift)
    M.push_model(ctx, cs, len(vs))
    key = (name, shift)
    if key not in _cache:
        _cache[key] = FC.oracle_model(vs, cs)
    lb0, ub0 = vs.bounds()
    return vs, _cache[key], lb0, ub0, mk


def oracle_tree(om, lb0, ub0, key, **kw):
    k = (key, tuple(sorted(kw.items())))
    if k not in _cache:
        _cache[k] = om.search(lb0, ub0, **kw)
    return _cache[k]


# ------------------------------------------------------------------------------------------------ 1. one tree is the reference
@pytest.mark.parametrize("steps", [1, 5, 64])
def test_one_tree_is_the_oracles_search(ctx, steps):
    vs, om, lb0, ub0, _ = case(ctx, "A4")
    want = FC.counts(oracle_tree(om, lb0, ub0, "A4", all_solutions=True)[0])
    assert want == (2025, 375, 638)
    r = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=steps, capacity=64, formulas=True)
    print("A4 one tree", steps, FC.counts(r), r["error"], r["open"])
    plan = ctx.last_plan()
    assert plan["path"] == 3 and plan["grid"] == 1 and plan["block"] == 256
    assert r["error"] == 0 and r["open"] == 0 and FC.counts(r) == want
    ss1, _, _, sol1 = oracle_tree(om, lb0, ub0, "A4", all_solutions=False)
    one = ctx.dfs_forest(lb0[None], ub0[None], stop_on_solution=True, want_solution=True, steps_per_launch=steps, capacity=64, formulas=True)
    print("A4 first solution", steps, FC.counts(one))
    assert FC.counts(one) == FC.counts(ss1) and ss1["num_nodes"] == 32
    assert np.array_equal(one["first_solutions"][0], sol1)


@pytest.mark.parametrize("k", [1, 7, 40])
def test_one_tree_leaves_what_dfs_device_leaves(ctx, k):
    """After k nodes: the counters, the open nodes and the stack rows [0, sp) of pcp_dfs_device, whatever the launch length."""
    vs, om, lb0, ub0, _ = case(ctx, "A4")
    ref_info = {}
    ref = ctx.dfs_device(lb0, ub0, 100000, capacity=64, stop_on_solution=False, node_limit=k, chunk=16, info=ref_info)
    for steps in (1, 5, 64):
        info = {}
        r = ctx.dfs_forest(lb0[None], ub0[None], node_limit_per_tree=k, steps_per_launch=steps, capacity=64, formulas=True, info=info)
        print("A4 after", k, "nodes, launches of", steps, FC.counts(r), r["open"], "| dfs_device", FC.counts(ref), ref["open"])
        assert FC.counts(r) == FC.counts(ref) and r["nodes"] == k and r["open"] == ref["open"] and r["error"] == ref["error"] == 0
        assert np.array_equal(info["rows"][0][0], ref_info["rows"][0]) and np.array_equal(info["rows"][0][1], ref_info["rows"][1])


def test_more_than_64_slots_and_units(ctx):
    vs, om, lb0, ub0, _ = case(ctx, "six")
    assert len(vs) > 64 and ctx.n_units > 64
    want = FC.counts(oracle_tree(om, lb0, ub0, "six", all_solutions=True, node_limit=3000)[0])
    r = ctx.dfs_forest(lb0[None], ub0[None], node_limit_per_tree=3000, steps_per_launch=512, capacity=128, formulas=True)
    print("six tasks", FC.counts(r), want)
    assert r["error"] == 0 and FC.counts(r) == want and want[0] == 3000


# ------------------------------------------------------------------------------------------------ 2. random formula stores
@pytest.mark.parametrize("seed", range(9000, 9006))
def test_random_formula_stores(ctx, seed):
    vs, cs = random_formula_store(seed)
    om = FC.oracle_model(vs, cs)
    M.push_model(ctx, cs, len(vs))
    lb0, ub0 = vs.bounds()
    want = FC.counts(om.search(lb0, ub0, all_solutions=True, node_limit=2000)[0])
    r = ctx.dfs_forest(lb0[None], ub0[None], node_limit_per_tree=2000, steps_per_launch=256, capacity=256, formulas=True)
    print("random store", seed, FC.counts(r), want)
    assert r["error"] == 0 and FC.counts(r) == want


# ------------------------------------------------------------------------------------------------ 3. expansion plus forest
@pytest.mark.parametrize("trees", [3, 5, 64])
def test_expansion_plus_forest_is_the_complete_tree(ctx, trees):
    from pcp_amd.search_forest import forest_search
    vs, om, lb0, ub0, _ = case(ctx, "A4")
    want = FC.counts(oracle_tree(om, lb0, ub0, "A4", all_solutions=True)[0])
    r = forest_search(ctx, lb0, ub0, n_trees=trees, steps_per_launch=16, capacity=64, formulas=True)
    plan = ctx.last_plan()
    print("A4 forest", trees, FC.counts(r), "trees", r["trees"], "grid", plan["grid"])
    assert r["error"] == 0 and FC.counts(r) == want and r["trees"] >= trees
    assert plan["path"] == 3 and plan["block"] == 256 and plan["grid"] == -(-r["trees"] // 4)
    parts = [forest_search(ctx, lb0, ub0, n_trees=trees, steps_per_launch=16, capacity=64, rank=k, world=2, formulas=True) for k in (0, 1)]
    assert tuple(sum(x) for x in zip(*(FC.counts(p) for p in parts))) == want


# ------------------------------------------------------------------------------------------------ 4. refill and growth
def test_refill_and_growth(ctx):
    from pcp_amd.search_forest import seed_roots_interval
    vs, om, lb0, ub0, _ = case(ctx, "A4")
    want = FC.counts(oracle_tree(om, lb0, ub0, "A4", all_solutions=True)[0])
    rl, ru, st = seed_roots_interval(ctx, lb0, ub0, 4)
    rest = (want[0] - st.num_nodes, want[1] - st.num_solution, want[2] - st.num_failed_node)
    r = ctx.dfs_forest(rl, ru, steps_per_launch=6, capacity=64, formulas=True)
    plain = ctx.dfs_forest(rl, ru, steps_per_launch=6, capacity=64, rebalance=False, formulas=True)
    print("refill", FC.counts(r), r["steals"], r["launches"], "| without", FC.counts(plain), plain["launches"])
    assert r["error"] == 0 and r["open"] == 0 and FC.counts(r) == rest and r["steals"] > 0
    assert FC.counts(plain) == rest and plain["steals"] == 0 and r["launches"] < plain["launches"]
    # stacks that start at two rows grow; a ceiling of two rows is reported as error 1
    info = {}
    g = ctx.dfs_forest(rl, ru, steps_per_launch=50, capacity=2, max_capacity=256, info=info, formulas=True)
    print("growth", FC.counts(g), info["grown"], info["capacity"])
    assert g["error"] == 0 and g["open"] == 0 and FC.counts(g) == rest and info["grown"] >= 1 and 2 < info["capacity"] <= 256
    low = ctx.dfs_forest(rl, ru, steps_per_launch=50, capacity=2, max_capacity=2, rebalance=False, formulas=True)
    assert low["error"] == 1 and low["open"] > 0
    # a tree that starts with an empty stack next to working trees
    import torch
    k = rl.shape[0]
    rl1, ru1 = torch.cat([rl, rl[:1]]), torch.cat([ru, ru[:1]])
    e = ctx.dfs_forest(rl1, ru1, steps_per_launch=64, capacity=64, sp0=[1] * k + [0], rebalance=False, formulas=True)
    assert e["error"] == 0 and e["open"] == 0 and FC.counts(e) == rest and e["per_tree"][k, 0] == 0


# ------------------------------------------------------------------------------------------------ 5. edge roots
def test_edge_roots_in_one_launch(ctx):
    vs, om, lb0, ub0, _ = case(ctx, "A4")
    want = FC.counts(oracle_tree(om, lb0, ub0, "A4", all_solutions=True)[0])
    sol = oracle_tree(om, lb0, ub0, "A4", all_solutions=False)[3]
    L = np.stack([lb0, sol, lb0, lb0]).astype(np.int32)
    U = np.stack([ub0, sol, ub0, ub0]).astype(np.int32)
    L[0, 0], U[0, 0] = 3, 2                      # an empty root
    assert FC.counts(om.search(L[1], U[1], all_solutions=True)[0]) == (1, 1, 0)  # a root that is a solution
    U[2, 1] = BOUND_MAX + 1                      # a bound beyond +-(2^29 - 1)
    r = ctx.dfs_forest(L, U, steps_per_launch=4096, capacity=64, max_launches=1, want_solution=True, formulas=True)
    pt = r["per_tree"]
    print("edge roots", pt.tolist())
    assert pt[0, :4].tolist() == [1, 0, 1, 0] and pt[1, :4].tolist() == [1, 1, 0, 0] and np.array_equal(r["first_solutions"][1], sol)
    assert pt[2, :4].tolist() == [1, 0, 0, 2] and r["error"] == 2
    assert tuple(pt[3, :3].tolist()) == want and pt[3, 3] == 0 and r["open"] == 0
    import pcp_amd.engine as E
    with pytest.raises(E.PcpError) as e:  # the refused root raised the sticky hull-violation word; reading it reports and clears it
        ctx.stats_read()
    assert e.value.code == -2
    ctx.stats_read()


def test_values_at_and_below_zero(ctx):
    """Start windows -3..2: MiddleVal of (-1, 0) is 0, not -1 — (lb + ub) / 2 truncates toward zero, so the left child `x <= 0` is its
    parent again and the reference descends for ever (the oracle does: 200 nodes, no leaf).  A device that rounded down would find leaves.
    The open rows are those pcp_dfs_device leaves."""
    vs, om, lb0, ub0, _ = case(ctx, "A4", shift=-3)
    assert lb0[0] == -3 and ub0[0] == 2
    want = FC.counts(oracle_tree(om, lb0, ub0, "A4-3", all_solutions=True, node_limit=200)[0])
    assert want == (200, 0, 0)
    info, ref_info = {}, {}
    r = ctx.dfs_forest(lb0[None], ub0[None], node_limit_per_tree=200, steps_per_launch=64, capacity=256, formulas=True, info=info)
    ref = ctx.dfs_device(lb0, ub0, 100000, capacity=256, stop_on_solution=False, node_limit=200, chunk=64, info=ref_info)
    print("A4 at -3..2", FC.counts(r), r["open"], want, "| dfs_device", FC.counts(ref), ref["open"])
    assert r["error"] == 0 and FC.counts(r) == want == FC.counts(ref) and r["open"] == ref["open"]
    assert np.array_equal(info["rows"][0][0], ref_info["rows"][0]) and np.array_equal(info["rows"][0][1], ref_info["rows"][1])


# ------------------------------------------------------------------------------------------------ 6. branch and bound
@pytest.mark.parametrize("name,mode", [("C4mk", "min"), ("C4mk", "max"), ("D5mk", "min"), ("D5mk", "max")])
def test_one_tree_of_branch_and_bound_is_the_host_specification(ctx, name, mode):
    vs, om, lb0, ub0, mk = case(ctx, name)
    want = S.dfs(ctx, lb0, ub0, objective=(mk, mode), batch=1)
    r = ctx.dfs_forest_bnb(lb0[None], ub0[None], (mk, mode), steps_per_launch=64, capacity=64)
    print(name, mode, FC.counts(r), r["best"], "| host", FC.counts(want), want.best)
    assert ctx.last_plan()["path"] == 3
    assert r["error"] == 0 and r["open"] == 0 and FC.counts(r) == FC.counts(want)
    assert r["best"] == want.best and int(r["best_solution"][mk]) == want.best and FC.is_schedule(name, r["best_solution"])
    assert want.best == {("C4mk", "min"): 5, ("C4mk", "max"): 12, ("D5mk", "min"): 7, ("D5mk", "max"): 14}[(name, mode)]


@pytest.mark.parametrize("trees", [3, 64])
def test_a_forest_of_branch_and_bound_finds_the_optimum(ctx, trees):
    from pcp_amd.search_forest import forest_bnb
    for name, mode, best in (("C4mk", "min", 5), ("C4mk", "max", 12), ("D5mk", "min", 7)):
        vs, om, lb0, ub0, mk = case(ctx, name)
        r = forest_bnb(ctx, lb0, ub0, (mk, mode), n_trees=trees, steps_per_launch=32, capacity=64)
        print(name, mode, trees, FC.counts(r), r["best"])
        assert r["error"] == 0 and r["open"] == 0 and r["best"] == best
        row = np.asarray(r["best_solution"], np.int32)
        assert int(row[mk]) == best and FC.is_schedule(name, row)
        status = ctx.propagate(row[None], row[None], None)[3]
        assert int(status[0]) == M.TRUE
    # an incumbent that is already the optimum: nothing beats it
    vs, om, lb0, ub0, mk = case(ctx, "C4mk")
    r = forest_bnb(ctx, lb0, ub0, (mk, "min"), n_trees=trees, steps_per_launch=32, capacity=64, best0=5)
    assert r["error"] == 0 and r["best"] is None and r["best_solution"] is None
    one = ctx.dfs_forest_bnb(lb0[None], ub0[None], (mk, "min"), best0=5, steps_per_launch=64, capacity=64)
    assert one["error"] == 0 and one["open"] == 0 and one["solutions"] == 0 and one["best"] is None


# ------------------------------------------------------------------------------------------------ 7. contract
def test_contract(ctx):
    import pcp_amd.engine as E
    vs, om, lb0, ub0, mk = case(ctx, "C4mk")
    V = len(vs)
    with pytest.raises(E.PcpError) as e:
        ctx.dfs_forest_bnb(lb0[None], ub0[None], (V, "min"), capacity=16)   # var >= n_vars
    assert e.value.code == -1
    r = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=0, max_launches=1, capacity=16, formulas=True)  # n_steps = 0: PCP_OK, nothing runs
    assert (r["nodes"], r["open"], r["error"]) == (0, 1, 0)
    # a store without formula units
    props = M.lower_units([M.XNeqY(M.Identity(0), M.Identity(1)), M.XLessY(M.Identity(2), M.Identity(3))], 4)
    ctx.set_model(4, props)
    with pytest.raises(E.PcpError) as e:
        ctx.dfs_forest(np.zeros((2, 4), np.int32), np.full((2, 4), 5, np.int32), capacity=16, formulas=True)
    assert e.value.code == -5 and "pcp_dfs_device" in str(e.value)
    # a set-mode model
    ctx.set_model(4, props, set_words=1)
    ctx.set_hull(0, 5)
    with pytest.raises(E.PcpError) as e:
        ctx.dfs_forest(np.zeros((2, 4), np.int32), np.full((2, 4), 5, np.int32), capacity=16, formulas=True)
    assert e.value.code == -1
