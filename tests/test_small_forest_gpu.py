"""The search forest over small Interval stores of plain propagators on the device (pcp_dfs_forest_device_small, _small_bnb;
pcp_smalldfs.hip): one tree against the oracle and against pcp_dfs_device node for node, mixed-kind stores at the kernel's edges,
expansion plus forest against the oracle's complete tree, refill and growth, edge roots in one workgroup, MiddleVal below zero, branch and
bound against the host specification, the all-XNeqY forest beside it, and the contract.  The models are those of small_forest_cases.py;
test_small_forest_cpu.py pins the figures the oracle and the host specification give on them."""
import ctypes as C_

import numpy as np
import pytest

import form_forest_cases as FC
import small_forest_cases as C
from pcp_amd import model as M
from pcp_amd import search as S
from test_small_forest_cpu import GOLOMB_BNB, GOLOMB_FIRST, GOLOMB_TREE, QUEENS8, STORE_TREE

pytestmark = pytest.mark.gpu

BOUND_MAX = (1 << 29) - 1


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


_cache = {}


def push(ctx, key, vs, cs):
    """Push the model; the oracle's model is built once per key."""
    M.push_model(ctx, cs, len(vs))
    if key not in _cache:
        _cache[key] = FC.oracle_model(vs, cs)
    lb0, ub0 = vs.bounds()
    return _cache[key], lb0, ub0


def golomb(ctx, m):
    vs, cs, var = C.golomb(m)
    return push(ctx, ("golomb", m), vs, cs) + (var,)


def oracle_tree(om, lb0, ub0, key, **kw):
    k = (key, tuple(sorted(kw.items())))
    if k not in _cache:
        _cache[k] = om.search(lb0, ub0, **kw)
    return _cache[k]


# ------------------------------------------------------------------------------------------------ 1. one tree is the reference
@pytest.mark.parametrize("steps", [1, 5, 64])
def test_one_tree_is_the_oracles_search(ctx, steps):
    om, lb0, ub0, _ = golomb(ctx, 5)
    want = FC.counts(oracle_tree(om, lb0, ub0, "g5", all_solutions=True)[0])
    assert want == GOLOMB_TREE[5]
    r = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=steps, capacity=64, small=True)
    print("golomb 5 one tree", steps, FC.counts(r), r["error"], r["open"])
    plan = ctx.last_plan()
    assert plan["path"] == 4 and plan["grid"] == 1 and plan["block"] == 256
    assert r["error"] == 0 and r["open"] == 0 and FC.counts(r) == want
    ss1, _, _, sol1 = oracle_tree(om, lb0, ub0, "g5", all_solutions=False)
    one = ctx.dfs_forest(lb0[None], ub0[None], stop_on_solution=True, want_solution=True, steps_per_launch=steps, capacity=64, small=True)
    print("golomb 5 first solution", steps, FC.counts(one))
    assert FC.counts(one) == FC.counts(ss1) == GOLOMB_FIRST[5][0]
    assert np.array_equal(one["first_solutions"][0], sol1)


@pytest.mark.parametrize("k", [1, 7, 40])
def test_one_tree_leaves_what_dfs_device_leaves(ctx, k):
    """After k nodes: the counters, the open nodes and the stack rows [0, sp) of pcp_dfs_device, whatever the launch length."""
    om, lb0, ub0, _ = golomb(ctx, 5)
    ref_info = {}
    ref = ctx.dfs_device(lb0, ub0, 100000, capacity=64, stop_on_solution=False, node_limit=k, chunk=16, info=ref_info)
    for steps in (1, 5, 64):
        info = {}
        r = ctx.dfs_forest(lb0[None], ub0[None], node_limit_per_tree=k, steps_per_launch=steps, capacity=64, small=True, info=info)
        print("golomb 5 after", k, "nodes, launches of", steps, FC.counts(r), r["open"], "| dfs_device", FC.counts(ref), ref["open"])
        assert FC.counts(r) == FC.counts(ref) and r["nodes"] == k and r["open"] == ref["open"] and r["error"] == ref["error"] == 0
        assert np.array_equal(info["rows"][0][0], ref_info["rows"][0]) and np.array_equal(info["rows"][0][1], ref_info["rows"][1])


# ------------------------------------------------------------------------------------------------ 3. mixed-kind stores
@pytest.mark.parametrize("name", sorted(C.STORES))
def test_stores_against_the_oracle(ctx, name):
    """Ternary kinds, constants, a Sum view and an XEqYMulZ (six seeds); two Distinct units; a Distinct beyond the 128-value mask; one of
    exactly 64 variables; more than 64 units; exactly 128 slots; exactly 2048 records."""
    vs, cs = C.store(name)
    om, lb0, ub0 = push(ctx, name, vs, cs)
    want = FC.counts(oracle_tree(om, lb0, ub0, name, all_solutions=True, node_limit=C.NODE_LIMIT)[0])
    assert want == STORE_TREE[name]
    r = ctx.dfs_forest(lb0[None], ub0[None], node_limit_per_tree=C.NODE_LIMIT, steps_per_launch=256, capacity=512, small=True)
    print("store", name, FC.counts(r), want, ctx.last_plan())
    assert ctx.last_plan()["path"] == 4
    assert r["error"] == 0 and FC.counts(r) == want


def test_a_distinct_pair_by_pair_gives_the_same_tree(ctx):
    vs, cs = C.store("distinct64")
    om, lb0, ub0 = push(ctx, "distinct64", vs, cs)
    try:
        ctx.set_option("small_alldiff", 0)
        r = ctx.dfs_forest(lb0[None], ub0[None], node_limit_per_tree=C.NODE_LIMIT, steps_per_launch=256, capacity=512, small=True)
    finally:
        ctx.set_option("small_alldiff", 1)
    print("distinct64 pair by pair", FC.counts(r))
    assert r["error"] == 0 and FC.counts(r) == STORE_TREE["distinct64"]


# ------------------------------------------------------------------------------------------------ 4. expansion plus forest
@pytest.mark.parametrize("trees", [3, 5, 64])
def test_expansion_plus_forest_is_the_complete_tree(ctx, trees):
    """3 and 5 trees leave a workgroup with idle wavefronts behind the kernel's barrier."""
    from pcp_amd.search_forest import forest_search
    om, lb0, ub0, _ = golomb(ctx, 5)
    want = GOLOMB_TREE[5]
    r = forest_search(ctx, lb0, ub0, n_trees=trees, steps_per_launch=16, capacity=64, small=True)
    plan = ctx.last_plan()
    print("golomb 5 forest", trees, FC.counts(r), "trees", r["trees"], "grid", plan["grid"])
    assert r["error"] == 0 and FC.counts(r) == want and r["trees"] >= trees
    assert plan["path"] == 4 and plan["block"] == 256 and plan["grid"] == -(-r["trees"] // 4)
    parts = [forest_search(ctx, lb0, ub0, n_trees=trees, steps_per_launch=16, capacity=64, rank=k, world=2, small=True) for k in (0, 1)]
    assert tuple(sum(x) for x in zip(*(FC.counts(p) for p in parts))) == want


def test_a_workgroup_with_three_trees(ctx):
    """Exactly three roots: the fourth wavefront of the only workgroup has no tree and must still pass the barrier."""
    from pcp_amd.search_forest import seed_roots_interval
    om, lb0, ub0, _ = golomb(ctx, 5)
    rl, ru, st = seed_roots_interval(ctx, lb0, ub0, 3)
    rl, ru = rl[:3], ru[:3]
    want = [FC.counts(om.search(rl[t].cpu().numpy(), ru[t].cpu().numpy(), all_solutions=True)[0]) for t in range(3)]
    r = ctx.dfs_forest(rl, ru, steps_per_launch=4096, capacity=64, rebalance=False, small=True)
    plan = ctx.last_plan()
    assert plan["grid"] == 1 and plan["block"] == 256
    assert r["error"] == 0 and r["open"] == 0 and [tuple(r["per_tree"][t, :3].tolist()) for t in range(3)] == want


# ------------------------------------------------------------------------------------------------ 5. refill and growth
def test_refill_and_growth(ctx):
    from pcp_amd.search_forest import seed_roots_interval
    om, lb0, ub0, _ = golomb(ctx, 5)
    want = GOLOMB_TREE[5]
    rl, ru, st = seed_roots_interval(ctx, lb0, ub0, 4)
    rest = (want[0] - st.num_nodes, want[1] - st.num_solution, want[2] - st.num_failed_node)
    r = ctx.dfs_forest(rl, ru, steps_per_launch=6, capacity=64, small=True)
    plain = ctx.dfs_forest(rl, ru, steps_per_launch=6, capacity=64, rebalance=False, small=True)
    print("refill", FC.counts(r), r["steals"], r["launches"], "| without", FC.counts(plain), plain["launches"])
    assert r["error"] == 0 and r["open"] == 0 and FC.counts(r) == rest and r["steals"] > 0
    assert FC.counts(plain) == rest and plain["steals"] == 0 and r["launches"] < plain["launches"]
    # stacks that start at two rows grow; a ceiling of two rows is reported as error 1
    info = {}
    g = ctx.dfs_forest(rl, ru, steps_per_launch=50, capacity=2, max_capacity=256, info=info, small=True)
    print("growth", FC.counts(g), info["grown"], info["capacity"])
    assert g["error"] == 0 and g["open"] == 0 and FC.counts(g) == rest and info["grown"] >= 1 and 2 < info["capacity"] <= 256
    low = ctx.dfs_forest(rl, ru, steps_per_launch=50, capacity=2, max_capacity=2, rebalance=False, small=True)
    assert low["error"] == 1 and low["open"] > 0
    # a tree that starts with an empty stack next to working trees, in the same workgroup: three roots and the empty one
    import torch
    rl3, ru3 = rl[:3], ru[:3]
    alone = ctx.dfs_forest(rl3, ru3, steps_per_launch=64, capacity=64, rebalance=False, small=True)
    rl1, ru1 = torch.cat([rl3[:1], rl3[:1], rl3[1:]]), torch.cat([ru3[:1], ru3[:1], ru3[1:]])
    e = ctx.dfs_forest(rl1, ru1, steps_per_launch=64, capacity=64, sp0=[1, 0, 1, 1], rebalance=False, small=True)
    assert ctx.last_plan()["grid"] == 1
    assert e["error"] == 0 and e["open"] == 0 and FC.counts(e) == FC.counts(alone) and e["per_tree"][1, 0] == 0
    assert np.array_equal(e["per_tree"][[0, 2, 3], :3], alone["per_tree"][:, :3])


# ------------------------------------------------------------------------------------------------ 6. edge roots
def test_edge_roots_in_one_launch(ctx):
    """All four in one workgroup."""
    om, lb0, ub0, _ = golomb(ctx, 5)
    want = GOLOMB_TREE[5]
    sol = oracle_tree(om, lb0, ub0, "g5", all_solutions=False)[3]
    L = np.stack([lb0, sol, lb0, lb0]).astype(np.int32)
    U = np.stack([ub0, sol, ub0, ub0]).astype(np.int32)
    L[0, 1], U[0, 1] = 3, 2                      # an empty root
    assert FC.counts(om.search(L[1], U[1], all_solutions=True)[0]) == (1, 1, 0)  # a root that is a solution
    U[2, 1] = BOUND_MAX + 1                      # a bound of 2^29
    r = ctx.dfs_forest(L, U, steps_per_launch=4096, capacity=64, max_launches=1, want_solution=True, small=True)
    pt = r["per_tree"]
    print("edge roots", pt.tolist())
    assert ctx.last_plan()["grid"] == 1 and ctx.last_plan()["block"] == 256
    assert pt[0, :4].tolist() == [1, 0, 1, 0] and pt[1, :4].tolist() == [1, 1, 0, 0] and np.array_equal(r["first_solutions"][1], sol)
    assert pt[2, :4].tolist() == [1, 0, 0, 2] and r["error"] == 2
    assert tuple(pt[3, :3].tolist()) == want and pt[3, 3] == 0 and r["open"] == 0
    import pcp_amd.engine as E
    with pytest.raises(E.PcpError) as e:  # the refused root raised the sticky hull-violation word; reading it reports and clears it
        ctx.stats_read()
    assert e.value.code == -2
    ctx.stats_read()


# ------------------------------------------------------------------------------------------------ 7. MiddleVal below zero
def test_marks_below_zero(ctx):
    """Marks from -3: MiddleVal of (-1, 0) is 0, not -1 — (lb + ub) / 2 truncates toward zero — so the reference descends for ever (the
    oracle does: 200 nodes, no leaf).  A device that rounded down would find leaves.  The open rows are those pcp_dfs_device leaves."""
    vs, cs = C.golomb_shifted(5, -3)
    om, lb0, ub0 = push(ctx, "g5-3", vs, cs)
    want = FC.counts(oracle_tree(om, lb0, ub0, "g5-3", all_solutions=True, node_limit=200)[0])
    assert want == (200, 0, 0)
    info, ref_info = {}, {}
    r = ctx.dfs_forest(lb0[None], ub0[None], node_limit_per_tree=200, steps_per_launch=64, capacity=256, small=True, info=info)
    ref = ctx.dfs_device(lb0, ub0, 100000, capacity=256, stop_on_solution=False, node_limit=200, chunk=64, info=ref_info)
    print("golomb 5 from -3", FC.counts(r), r["open"], want, "| dfs_device", FC.counts(ref), ref["open"])
    assert r["error"] == 0 and FC.counts(r) == want == FC.counts(ref) and r["open"] == ref["open"]
    assert np.array_equal(info["rows"][0][0], ref_info["rows"][0]) and np.array_equal(info["rows"][0][1], ref_info["rows"][1])


# ------------------------------------------------------------------------------------------------ 8. branch and bound
@pytest.mark.parametrize("m,mode", sorted(GOLOMB_BNB))
def test_one_tree_of_branch_and_bound_is_the_host_specification(ctx, m, mode):
    om, lb0, ub0, var = golomb(ctx, m)
    want = S.dfs(ctx, lb0, ub0, objective=(var, mode), batch=1)
    assert (want.best, FC.counts(want)) == GOLOMB_BNB[(m, mode)]
    r = ctx.dfs_forest_bnb(lb0[None], ub0[None], (var, mode), steps_per_launch=64, capacity=64, small=True)
    print("golomb", m, mode, FC.counts(r), r["best"], "| host", FC.counts(want), want.best)
    assert ctx.last_plan()["path"] == 4
    assert r["error"] == 0 and r["open"] == 0 and FC.counts(r) == FC.counts(want)
    assert r["best"] == want.best and int(r["best_solution"][var]) == want.best and C.is_ruler(r["best_solution"], m)


@pytest.mark.parametrize("trees", [3, 64])
def test_a_forest_of_branch_and_bound_finds_the_optimum(ctx, trees):
    from pcp_amd.search_forest import forest_bnb
    for m in (5, 6):
        om, lb0, ub0, var = golomb(ctx, m)
        r = forest_bnb(ctx, lb0, ub0, (var, "min"), n_trees=trees, steps_per_launch=32, capacity=64, small=True)
        print("golomb", m, trees, FC.counts(r), r["best"])
        assert r["error"] == 0 and r["open"] == 0 and r["best"] == C.OPTIMUM[m] == {5: 11, 6: 17}[m]
        row = np.asarray(r["best_solution"], np.int32)
        assert int(row[var]) == C.OPTIMUM[m] and C.is_ruler(row, m)
        status = ctx.propagate(row[None], row[None], None)[3]
        assert int(status[0]) == M.TRUE
    # an incumbent that is already the optimum: nothing beats it
    om, lb0, ub0, var = golomb(ctx, 5)
    r = forest_bnb(ctx, lb0, ub0, (var, "min"), n_trees=trees, steps_per_launch=32, capacity=64, best0=11, small=True)
    assert r["error"] == 0 and r["best"] is None and r["best_solution"] is None
    one = ctx.dfs_forest_bnb(lb0[None], ub0[None], (var, "min"), best0=11, steps_per_launch=64, capacity=64, small=True)
    assert one["error"] == 0 and one["open"] == 0 and one["solutions"] == 0 and one["best"] is None


# ------------------------------------------------------------------------------------------------ 9. two forests, one tree
def test_queens8_through_both_forests(ctx):
    vs, cs = C.queens8()
    om, lb0, ub0 = push(ctx, "queens8", vs, cs)
    small = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=256, capacity=64, small=True)
    assert ctx.last_plan()["path"] == 4
    neq = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=256, capacity=64)
    assert ctx.last_plan()["path"] == 1
    print("queens 8", FC.counts(small), FC.counts(neq))
    assert small["error"] == neq["error"] == 0 and FC.counts(small) == FC.counts(neq) == QUEENS8 and QUEENS8[1] == 92


# ------------------------------------------------------------------------------------------------ 10. contract
def test_contract(ctx):
    import pcp_amd.engine as E
    om, lb0, ub0, var = golomb(ctx, 5)
    V = len(lb0)
    with pytest.raises(E.PcpError) as e:
        ctx.dfs_forest_bnb(lb0[None], ub0[None], (V, "min"), capacity=16, small=True)   # var >= n_vars
    assert e.value.code == -1
    r = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=0, max_launches=1, capacity=16, small=True)  # n_steps = 0: PCP_OK, nothing runs
    assert (r["nodes"], r["open"], r["error"]) == (0, 1, 0)

    # the objective struct: a bad mode, a null best, a null tree_best — straight at the C entry
    import torch
    dev = torch.device("cuda", ctx.device)
    lb = torch.zeros((1, 16, V), dtype=torch.int32, device=dev)
    ub = torch.zeros((1, 16, V), dtype=torch.int32, device=dev)
    sp, stop = torch.ones(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    status, counters = torch.zeros((1, 16), dtype=torch.uint8, device=dev), torch.zeros((1, 5), dtype=torch.int64, device=dev)
    best, tbest = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    st = E.DfsState(lb.data_ptr(), ub.data_ptr(), 16, sp.data_ptr(), stop.data_ptr(), status.data_ptr(), counters.data_ptr(), None, None)
    call = lambda obj: ctx._L.pcp_dfs_forest_device_small_bnb(ctx._h, C_.byref(st), 1, C_.byref(obj) if obj is not None else None, 0, 0, None)
    assert call(E.ForestObjective(var, 0, best.data_ptr(), tbest.data_ptr(), None)) == 0       # (n_steps = 0, `dirty` NULL: accepted)
    assert call(E.ForestObjective(var, 2, best.data_ptr(), tbest.data_ptr(), None)) == -1
    assert call(E.ForestObjective(var, 0, None, tbest.data_ptr(), None)) == -1
    assert call(E.ForestObjective(var, 0, best.data_ptr(), None, None)) == -1
    assert call(None) == -1

    # the stores one step beyond the limits: 129 slots, 2049 records
    for f in (C.slots129, C.recs2049):
        vs, cs = f()
        M.push_model(ctx, cs, len(vs))
        l0, u0 = vs.bounds()
        with pytest.raises(E.PcpError) as e:
            ctx.dfs_forest(l0[None], u0[None], capacity=16, small=True)
        assert e.value.code == -5 and "pcp_dfs_device" in str(e.value) and "pcp_dfs_forest_device_small" in str(e.value)
    # a store with formula units
    vs, cs, _ = FC.schedule("A4")
    M.push_model(ctx, cs, len(vs))
    l0, u0 = vs.bounds()
    with pytest.raises(E.PcpError) as e:
        ctx.dfs_forest(l0[None], u0[None], capacity=16, small=True)
    assert e.value.code == -5 and "pcp_dfs_forest_device_form" in str(e.value)
    with pytest.raises(ValueError):
        ctx.dfs_forest(l0[None], u0[None], capacity=16, small=True, formulas=True)
    # a set-mode model
    props = M.lower_units([M.XNeqY(M.Identity(0), M.Identity(1)), M.XLessY(M.Identity(2), M.Identity(3))], 4)
    ctx.set_model(4, props, set_words=1)
    ctx.set_hull(0, 5)
    with pytest.raises(E.PcpError) as e:
        ctx.dfs_forest(np.zeros((2, 4), np.int32), np.full((2, 4), 5, np.int32), capacity=16, small=True)
    assert e.value.code == -1
    # the other interval forests keep refusing this store of plain propagators
    ctx.set_model(4, props)
    for kw in ({}, {"formulas": True}):
        with pytest.raises(E.PcpError) as e:
            ctx.dfs_forest(np.zeros((2, 4), np.int32), np.full((2, 4), 5, np.int32), capacity=16, **kw)
        assert e.value.code == -5 and "pcp_dfs_device" in str(e.value)
    r = ctx.dfs_forest(np.zeros((2, 4), np.int32), np.full((2, 4), 5, np.int32), capacity=16, small=True)  # ... and this one takes it
    assert r["error"] == 0 and r["open"] == 0 and r["solutions"] > 0
