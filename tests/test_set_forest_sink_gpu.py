"""The set solution sink on the GPU (-m gpu): trail_dfs<.., SINK> in setdfs_kernel (stores of records, a workgroup per tree) and
setformdfs_kernel (stores with formula units, a wavefront per tree) through pcp_set_solution_sink_set, against the brute-force solution
sets and the restatement of set_forest_sink_cases.py, which test_set_forest_sink_cpu.py pins — never against the code under test."""
import ctypes as C

import numpy as np
import pytest

from pcp_amd import model as M
from pcp_amd import search_forest as SF

import set_forest_sink_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


def push(ctx, name):
    """The model on the context; returns (root [1, V, sw], run = the driver of its forest, lb0, ub0, base)."""
    vs, cs = K.build(name)
    sw, base, hi, form = K.SHAPE[name]
    M.push_model(ctx, cs, len(vs), sw)
    ctx.set_hull(base, hi)
    lb0, ub0 = vs.bounds()
    return K.root_bits(name)[None], (ctx.dfs_forest_setform if form else ctx.dfs_forest_set), lb0, ub0, base


def counts(r):
    assert r["error"] == 0, r
    return r["nodes"], r["solutions"], r["failed"]


# ------------------------------------------------------------------------------------------------ 1. every solution, every model
@pytest.mark.parametrize("brancher,val", K.BRANCHERS)
@pytest.mark.parametrize("name", K.MODELS)
def test_every_solution_comes_back(ctx, name, brancher, val):
    """One tree from the hull, then five trees from seed_roots: with an ample sink the counters are those of the run without a sink and of
    the restatement, the rows are pairwise-disjoint products of solutions, their union is the brute-force set, and there is one row per
    counted solution.  (Fails before this change: no such keyword, no such symbol.)"""
    root, run, lb0, ub0, base = push(ctx, name)
    want = K.counts_of(name, brancher, val)
    plain = run(root, brancher=brancher, val=val)
    r = run(root, brancher=brancher, val=val, collect_solutions=True, sink_capacity=256)
    print(name, brancher, val, "one tree", counts(r), want)
    assert counts(r) == counts(plain) == want and not r["stopped"]
    assert len(r["solutions_bits"]) == r["solutions"] and (r["solution_tree"] == 0).all()
    K.check_products(name, r["solutions_bits"])
    assert K.multiset(r["solutions_bits"]) == K.multiset(K.reference(name, brancher, val)["sets"])
    # five trees: the expansion's own True nodes and the trees' rows together
    roots, st, found = SF.seed_roots(ctx, lb0, ub0, base, 5, brancher=brancher, val=val, collect_solutions=True)
    assert len(found) == st.num_solution
    if roots.shape[0] == 0:
        assert st.num_nodes == want[0]
        K.check_products(name, found)
        return
    plain = run(roots, brancher=brancher, val=val, steps_per_launch=16)
    r = run(roots, brancher=brancher, val=val, steps_per_launch=16, collect_solutions=True, sink_capacity=256)
    print(name, brancher, val, roots.shape[0], "trees", counts(r), "expansion", st.num_nodes, st.num_solution, st.num_failed_node)
    assert counts(r) == counts(plain)
    assert (st.num_nodes + r["nodes"], st.num_solution + r["solutions"], st.num_failed_node + r["failed"]) == want
    assert len(r["solutions_bits"]) == r["solutions"] and set(r["solution_tree"].tolist()) <= set(range(roots.shape[0]))
    K.check_products(name, np.concatenate([found, r["solutions_bits"]]))


# ------------------------------------------------------------------------------------------------ 2. hand-back
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("name,brancher,val,n_trees", [("rec4", "split", "middle", 1), ("rec4", "enumerate", "middle", 1),
                                                        ("form4", "split", "middle", 5), ("form4", "enumerate", "min", 5), ("rec3w", "split", "middle", 1)])
def test_full_sink_hands_nodes_back(ctx, name, brancher, val, n_trees, steps):
    """Sink capacities 1, 2, count - 1 and count: the counters and the multiset of rows are those of the ample run, no row twice, and the
    tickets drawn beyond the capacity, summed over the drains, are the nodes handed back.  rec4: a workgroup per tree; form4: a wavefront
    per tree, several trees of one workgroup, so that one tree's error 6 stops while its neighbours run on."""
    root, run, lb0, ub0, base = push(ctx, name)
    if n_trees > 1:
        root, _ = SF.seed_roots(ctx, lb0, ub0, base, n_trees, brancher=brancher, val=val)
        assert root.shape[0] >= n_trees
    kw = dict(brancher=brancher, val=val, steps_per_launch=steps, rebalance=False)
    ample = run(root, collect_solutions=True, sink_capacity=4096, **kw)
    n = ample["solutions"]
    assert ample["error"] == 0 and n == len(ample["solutions_bits"]) >= 4
    K.check_products(name, ample["solutions_bits"], complete=n_trees == 1)
    for cap in (1, 2, n - 1, n):
        info = {}
        r = run(root, collect_solutions=True, sink_capacity=cap, info=info, **kw)
        print(name, brancher, steps, "capacity", cap, counts(r), "drains", info["drains"], "handed back", info["handed_back"], "launches", r["launches"])
        assert counts(r) == counts(ample) and (r["per_tree"] == ample["per_tree"]).all()
        assert K.multiset(r["solutions_bits"]) == K.multiset(ample["solutions_bits"])
        assert len(set(K.multiset(r["solutions_bits"]))) == n
        # (a sink smaller than the solution count must fill: rows leave it only when it is full or the search is over)
        assert info["overdrawn"] == info["handed_back"] and (info["handed_back"] > 0) == (cap < n)


# ------------------------------------------------------------------------------------------------ 3. the raw entry
def test_five_trees_race_for_one_row(ctx):
    """One launch, five trees, a one-row sink attached by hand: the tickets are drawn atomically — exactly one tree gets the row and counts
    its solution, every other tree that found one holds error 6 with nothing counted, and the stop word is raised."""
    import torch
    import pcp_amd.engine as E
    root, run, lb0, ub0, base = push(ctx, "form4")
    roots, _ = SF.seed_roots(ctx, lb0, ub0, base, 5)
    T = roots.shape[0]
    sink = E.SetSolutionSink(1, ctx.n_vars, ctx.set_words, torch.device("cuda", 0))
    sink.bits.fill_(-1)
    ctx.set_solution_sink_set(sink)
    try:
        r = run(roots, steps_per_launch=64, max_launches=1, rebalance=False)
        drawn = int(sink.count.item())
    finally:
        ctx.set_solution_sink_set(None)
    full = r["per_tree"][:, 3] == E.SINK_FULL
    print("race", T, "trees, tickets", drawn, "per tree", r["per_tree"].tolist())
    assert drawn >= 2 and r["stopped"] and r["error"] == E.SINK_FULL
    assert r["solutions"] == 1 and full.sum() == drawn - 1
    assert sink.drain() == 1 and sink.overdrawn == drawn - 1
    bits, tree = sink.rows()
    winner = int(tree[0])
    assert r["per_tree"][winner, 1] == 1  # (it may hold error 6 as well: its NEXT solution found the sink full)
    K.check_products("form4", bits, complete=False)


def test_limit_node_draws_no_ticket(ctx):
    """StopNode's limit node is a True node (the limit is chosen from the restatement): it is a node and nothing else — no ticket, no row."""
    root, run, *_ = push(ctx, "rec4")
    n = K.limit_on_a_true_node("rec4")
    want = K.reference("rec4", node_limit=n)
    for steps in (256, 1):
        r = run(root, node_limit=n, steps_per_launch=steps, collect_solutions=True, sink_capacity=64)
        print("limit", n, steps, counts(r))
        assert counts(r) == (want["nodes"], want["solutions"], want["failed"]) and r["stopped"] and r["total_nodes"] == n
        assert K.multiset(r["solutions_bits"]) == K.multiset(want["sets"])


def test_stop_on_solution_with_a_one_row_sink(ctx):
    """Several trees, capacity 1, stop_on_solution: one row or more, one per counted solution, none lost; the trees that found the sink
    full keep uncounted open nodes of a stopped forest, and the error is 0."""
    root, run, lb0, ub0, base = push(ctx, "form4")
    roots, _ = SF.seed_roots(ctx, lb0, ub0, base, 5)
    r = run(roots, stop_on_solution=True, steps_per_launch=64, collect_solutions=True, sink_capacity=1)
    print("stop on solution", counts(r), r["launches"])
    assert r["stopped"] and r["error"] == 0 and r["solutions"] == len(r["solutions_bits"]) >= 1 and r["first_solution"] is not None
    K.check_products("form4", r["solutions_bits"], complete=False)


def test_a_tree_stopped_by_a_full_sink_is_an_ordinary_donor(ctx):
    """Two trees, the second idle: with a one-row sink and launches of 3 nodes tree 0 stops on error 6 again and again, and
    pcp_dfs_forest_split_set takes its oldest open right branch for tree 1 right behind such a stop.  The totals are the restatement's."""
    root, run, *_ = push(ctx, "rec4")
    roots = np.concatenate([root, np.zeros_like(root)])

    def launch(st, steps, stream):
        return ctx._L.pcp_dfs_forest_device_set(ctx._h, C.byref(st), steps, 0, 0, C.c_void_p(stream))

    info = {}
    r = ctx._run_forest_set(roots, launch, steps_per_launch=3, live=[True, False], collect=1, info=info)
    print("donor", counts(r), info)
    assert counts(r) == K.counts_of("rec4") and info["splits"] >= 1 and info["handed_back"] >= 1 and (r["per_tree"][:, 0] > 0).all()
    assert len(r["solutions_bits"]) == r["solutions"] and set(r["solution_tree"].tolist()) == {0, 1}
    K.check_products("rec4", r["solutions_bits"])


# ------------------------------------------------------------------------------------------------ 4. refusals and lifetime
def test_refusals_and_lifetime(ctx):
    import torch
    import pcp_amd.engine as E
    dev = torch.device("cuda", 0)
    root, run, *_ = push(ctx, "rec4")
    good = E.SetSolutionSink(1, 4, 1, dev)
    L, h = ctx._L, ctx._h

    def attach(bits=good.bits.data_ptr(), count=good.count.data_ptr(), capacity=1, reserved=0):
        st = E.PcpSetSolutionSink(bits, good.tree.data_ptr(), count, capacity, reserved)
        return L.pcp_set_solution_sink_set(h, C.byref(st))

    assert attach() == 0
    # malformed sinks: PCP_ERR_ARG, and the sink attached before stays — a run still hands back on error 6
    assert attach(bits=None) == attach(count=None) == attach(capacity=0) == attach(reserved=1) == -1
    r = run(root, max_launches=1)
    assert r["error"] == E.SINK_FULL and int(good.count.item()) == 2
    good.count.zero_()
    # both branch-and-bound entries refuse it, naming the sink, and run once it is detached
    with pytest.raises(E.PcpError) as e:
        ctx.dfs_forest_set_bnb(root, (0, "min"), steps_per_launch=64)
    assert e.value.code == -5 and "sink" in str(e.value) and "pcp_set_solution_sink_set" in str(e.value)
    assert L.pcp_set_solution_sink_set(h, None) == 0
    assert ctx.dfs_forest_set_bnb(root, (0, "min"), steps_per_launch=64)["best"] == 0
    with pytest.raises(ValueError, match="branch and bound"):
        ctx.dfs_forest_set_bnb(root, (0, "min"), collect_solutions=True)
    # with only the Interval sink attached the set entries still refuse (test_forest_sink_gpu.py is the authority)
    isink = E.SolutionSink(4, 4, dev)
    ctx.solution_sink_set(isink)
    try:
        with pytest.raises(E.PcpError) as e:
            run(root)
        assert e.value.code == -5 and "pcp_solution_sink_set" in str(e.value)
        with pytest.raises(E.PcpError):
            run(root, collect_solutions=True)  # ... and the set sink the driver attached is detached on the way out:
    finally:
        ctx.solution_sink_set(None)
    assert ctx.dfs_forest_set_bnb(root, (0, "min"), steps_per_launch=64)["best"] == 0  # (it would refuse a set sink left behind)
    assert counts(run(root)) == K.counts_of("rec4") and int(good.count.item()) == 0
    # pcp_model_reset detaches
    assert attach() == 0
    root, run, *_ = push(ctx, "rec4")
    assert counts(run(root)) == K.counts_of("rec4") and int(good.count.item()) == 0
    # the formula entry under branch and bound
    root, run, *_ = push(ctx, "form4")
    fs = E.SetSolutionSink(1, 4, 1, dev)
    ctx.set_solution_sink_set(fs)
    try:
        with pytest.raises(E.PcpError) as e:
            ctx.dfs_forest_setform_bnb(root, (0, "min"), steps_per_launch=64)
        assert e.value.code == -5 and "sink" in str(e.value)
    finally:
        ctx.set_solution_sink_set(None)
    assert ctx.dfs_forest_setform_bnb(root, (0, "min"), steps_per_launch=64)["best"] == 0
    # an interval-mode context takes no set sink
    vs, cs = K.build("rec4")
    M.push_model(ctx, cs, len(vs), 0)
    assert attach() == -1 and b"set-mode" in L.pcp_last_error(h)
    push(ctx, "rec4")


# ------------------------------------------------------------------------------------------------ 5. expansion plus forest
@pytest.mark.parametrize("brancher,val", K.BRANCHERS)
@pytest.mark.parametrize("name", ["queens6", "sched4"])
def test_forest_search_set_returns_the_expansions_solutions_too(ctx, name, brancher, val):
    """Expansion rows (tree -1, first) plus forest rows cover the brute-force set exactly; formulas=True dispatches to the formula forest."""
    _, _, lb0, ub0, base = push(ctx, name)
    form = K.SHAPE[name][3]
    r = SF.forest_search_set(ctx, lb0, ub0, base, n_trees=6, steps_per_launch=8, brancher=brancher, val=val, formulas=form, collect_solutions=True, sink_capacity=3)
    print(name, brancher, val, counts(r), "trees", r["trees"], "seeded", r["seeded_solutions"])
    assert counts(r) == K.counts_of(name, brancher, val) and len(r["solutions_bits"]) == r["solutions"]
    k = r["seeded_solutions"]
    assert (r["solution_tree"][:k] == -1).all() and (r["solution_tree"][k:] >= 0).all()
    assert ctx.last_plan()["path"] == (3 if form else 0) or r["trees"] == 0
    K.check_products(name, r["solutions_bits"])
