"""The solution sink of the all-XNeqY forest on the device (pcp_dfs_forest_device_neq_sink; neqfix_kernel<.., DFS, .., SINK>, pcp_neq.hip):
every case of neq_forest_sink_cases.py under BinarySplit and both Enumerate selectors, with and without a declared hull — the boxes are
disjoint, their points are the brute-force set, and nodes / solutions / failed are those of the counting entries that were there before
(pcp_dfs_forest_device, pcp_dfs_forest_device_neq_enum) on the same root; a sink of 1, 2, count - 1 and count rows drained by hand through
the raw entry; several trees through forest_solutions, also at the tree count from which the launcher takes 128-thread workgroups;
stop_on_solution and the StopNode limit node; error 6 next to the exclusion path; the refusals of the C entry.

The search loop runs on int2 cells whether a hull is declared or not (launch_neq_dfs, pcp_api.hip), so the two hull cases run the same
instantiation; N-queens and the box model take the 4-byte adjacency payloads."""
import ctypes as C_
import os
import re

import numpy as np
import pytest

import neq_enum_forest_cases as NC
import neq_forest_sink_cases as NK
from pcp_amd import model as M
from test_neq_enum_forest_cpu import ENUM_TREE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = -1         # row_excl[r].var == 0xFFFFFFFF as int32
SENTINEL = -7777  # what a sink row holds before anything is written to it
BRANCHERS = {"split": ("split", "middle"), "enum-middle": ("enumerate", "middle"), "enum-min": ("enumerate", "min")}
QUEENS = {"queens6": 6, "queens8": 8}


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


def counts(r):
    return r["nodes"], r["solutions"], r["failed"]


def count_only(ctx, lb, ub, brancher, val, **kw):
    """The entries that were there before the sink, on the same roots: the reference of every counter."""
    lb, ub = np.atleast_2d(lb), np.atleast_2d(ub)
    if brancher == "split":
        return ctx.dfs_forest(lb, ub, **kw)
    return ctx.dfs_forest_enum(lb, ub, val=val, forest="neq", **kw)


class Raw:
    """The buffers of n trees, a sentinel-filled sink of `sink_rows` rows, and the C entry itself, one call per launch."""

    def __init__(self, ctx, lbs, ubs, brancher="split", val="middle", sink_rows=256, capacity=64, path_capacity=128):
        import torch
        import pcp_amd.engine as E
        self.E, self.ctx, self.torch = E, ctx, torch
        self.dev = torch.device("cuda", ctx.device)
        lbs, ubs = np.atleast_2d(lbs).astype(np.int32), np.atleast_2d(ubs).astype(np.int32)
        T, V = lbs.shape
        self.T, self.V, self.cap = T, V, capacity
        z = self.z
        self.lb, self.ub = z(T, capacity, V), z(T, capacity, V)
        self.lb[:, 0], self.ub[:, 0] = torch.from_numpy(lbs).to(self.dev), torch.from_numpy(ubs).to(self.dev)
        self.sp, self.stop = torch.ones(T, dtype=torch.int32, device=self.dev), z(T)
        self.status, self.counters = z(T, capacity, dt=torch.uint8), z(T, 5, dt=torch.int64)
        self.dirty = torch.full((T, capacity), -1, dtype=torch.int32, device=self.dev)
        self.enum = brancher == "enumerate"
        self.row_base, self.row_excl = z(T, capacity), z(T, capacity, 2)
        self.row_excl[:, :, 0] = NONE
        self.val = E.VAL_MODES[val]
        self.path, self.path_capacity = z(T, max(path_capacity, 1), 2), path_capacity
        self.rows = sink_rows
        self.s_lb = torch.full((sink_rows, V), SENTINEL, dtype=torch.int32, device=self.dev)
        self.s_ub = torch.full((sink_rows, V), SENTINEL, dtype=torch.int32, device=self.dev)
        self.s_tree = torch.full((sink_rows,), SENTINEL, dtype=torch.int32, device=self.dev)
        self.s_count = z(1)
        self.got_lb, self.got_ub, self.got_tree = [], [], []
        self.drains = 0

    def z(self, *s, dt=None):
        return self.torch.zeros(s, dtype=dt or self.torch.int32, device=self.dev)

    def call(self, n_steps, stop_on_solution=0, node_limit=0, st=True, sink=True, st_over=None, ex_over=None, sink_over=None):
        E = self.E
        s = E.DfsState(self.lb.data_ptr(), self.ub.data_ptr(), self.cap, self.sp.data_ptr(), self.stop.data_ptr(), self.status.data_ptr(), self.counters.data_ptr(),
                       None, self.dirty.data_ptr())
        x = E.ForestExcl(self.path.data_ptr() if self.path_capacity else None, self.row_base.data_ptr(), self.row_excl.data_ptr(), self.path_capacity, self.val)
        k = E.PcpSolutionSink(self.s_lb.data_ptr(), self.s_ub.data_ptr(), self.s_tree.data_ptr(), self.s_count.data_ptr(), self.rows, 0)
        for obj, over in ((s, st_over), (x, ex_over), (k, sink_over)):
            for name, v in (over or {}).items():
                setattr(obj, name, v)
        rc = self.ctx._L.pcp_dfs_forest_device_neq_sink(self.ctx._h, C_.byref(s) if st else None, self.T, C_.byref(x) if self.enum else None,
                                                        C_.byref(k) if sink else None, n_steps, stop_on_solution, node_limit, None)
        self.torch.cuda.synchronize()
        return rc

    def drain(self):
        """Copy the valid rows out by hand, check the untouched ones, refill with the sentinel, zero the count.  Returns (drawn, valid)."""
        drawn = int(self.s_count[0])
        n = min(drawn, self.rows)
        lb, ub, tree = self.s_lb.cpu().numpy(), self.s_ub.cpu().numpy(), self.s_tree.cpu().numpy()
        assert (lb[n:] == SENTINEL).all() and (ub[n:] == SENTINEL).all() and (tree[n:] == SENTINEL).all(), "rows past the valid ones were written"
        assert (lb[:n] != SENTINEL).all() and (ub[:n] != SENTINEL).all() and ((tree[:n] >= 0) & (tree[:n] < self.T)).all()
        self.got_lb += list(lb[:n].copy()); self.got_ub += list(ub[:n].copy()); self.got_tree += tree[:n].tolist()
        self.s_lb.fill_(SENTINEL); self.s_ub.fill_(SENTINEL); self.s_tree.fill_(SENTINEL); self.s_count.zero_()
        self.drains += 1
        return drawn, n

    def run_draining(self, n_steps, max_launches=1 << 12):
        """Launch until every tree is done; drain when a tree handed a node back (and at the end), and resume those trees.  Returns the
        hand-backs."""
        handed = 0
        for _ in range(max_launches):
            assert self.call(n_steps) == 0
            err = self.counters[:, 3].cpu().numpy()
            assert set(err.tolist()) <= {0, 6}, err
            full = np.nonzero(err == 6)[0]
            done = not len(full) and not ((self.sp > 0) & (self.stop == 0)).any()
            if len(full) or done:
                drawn, n = self.drain()
                assert drawn - n == len(full), (drawn, n, full)  # *count exceeds the capacity by exactly the handed-back nodes
                assert not len(full) or n == self.rows
            for t in full:
                assert int(self.stop[t]) == 1 and int(self.sp[t]) >= 1
                self.counters[t, 3] = 0
                self.stop[t] = 0
            handed += len(full)
            if done:
                break
        return handed


# ------------------------------------------------------------------------------------------------ 1. every case, one tree, an ample sink
@pytest.fixture(scope="module")
def reference(ctx):
    """Per (case, brancher key): counts of the counting entry from the root — computed once, without a hull."""
    out = {}
    for name in NK.CASES:
        lb0, ub0 = NK.push(ctx, name)
        for key, (brancher, val) in BRANCHERS.items():
            r = count_only(ctx, lb0, ub0, brancher, val, steps_per_launch=64, capacity=64)
            assert r["error"] == 0 and r["open"] == 0
            out[(name, key)] = counts(r)
    return out


@pytest.mark.parametrize("hull", [True, False], ids=["hull", "nohull"])
@pytest.mark.parametrize("key", sorted(BRANCHERS))
@pytest.mark.parametrize("name", NK.CASES)
def test_one_tree_returns_every_solution_and_counts_as_the_counting_entry(ctx, reference, name, key, hull):
    brancher, val = BRANCHERS[key]
    lb0, ub0 = NK.push(ctx, name, declare_hull=hull)
    info = {}
    r = ctx.dfs_forest_neq_solutions(lb0[None], ub0[None], brancher=brancher, val=val, sink_capacity=256, steps_per_launch=64, capacity=64, info=info)
    p = ctx.last_plan()
    assert p["path"] == 1 and p["grid"] == 1 and p["packed"] == 0 and p["block"] == 512
    proper = NK.check_boxes(name, r["solutions_lb"], r["solutions_ub"])
    print(name, key, hull, counts(r), reference[(name, key)], "rows", len(r["solutions_lb"]), "proper boxes", proper, "drains", info["drains"])
    assert r["error"] == 0 and r["open"] == 0 and info["drains"] == 0
    assert len(r["solutions_lb"]) == r["solutions"] == int(r["per_tree"][0, 1])
    assert (r["solution_tree"] == 0).all()
    assert counts(r) == reference[(name, key)]
    if name in QUEENS:
        n = QUEENS[name]
        assert counts(r) == (ENUM_TREE[(n, val)] if brancher == "enumerate" else ENUM_TREE[(n, "min")])  # (BinarySplit's tree of N-queens is MinVal's)
        assert proper == 0 and r["solutions"] == NK.N_SOLUTIONS[name]
    if name == "box":
        assert proper == r["solutions"] == 2  # two True nodes, four points each
    if name == "wide":
        assert r["solutions"] == 2 and (r["solutions_lb"][:, 4:] == lb0[4:]).all() and (r["solutions_ub"][:, 4:] == ub0[4:]).all()


# ------------------------------------------------------------------------------------------------ 2. small sinks, drained by hand
@pytest.mark.parametrize("key", ["split", "enum-middle"])
@pytest.mark.parametrize("name,rows", [("queens6", 1), ("queens6", 2), ("queens6", 3), ("queens6", 4), ("queens8", 1), ("queens8", 2), ("queens8", 91), ("queens8", 92)])
def test_a_small_sink_drained_by_hand_loses_and_repeats_nothing(ctx, reference, name, rows, key):
    brancher, val = BRANCHERS[key]
    lb0, ub0 = NK.push(ctx, name)
    raw = Raw(ctx, lb0, ub0, brancher, val, sink_rows=rows)
    handed = raw.run_draining(7 if name == "queens6" else 61)
    cn = raw.counters.cpu().numpy()[0]
    print(name, key, "sink rows", rows, "counters", cn.tolist(), "handed back", handed, "drains", raw.drains)
    assert tuple(cn[:3].tolist()) == reference[(name, key)] and cn[3] == 0 and int(raw.sp[0]) == 0
    assert len(raw.got_lb) == NK.N_SOLUTIONS[name] == cn[1]
    assert NK.check_boxes(name, raw.got_lb, raw.got_ub) == 0  # exact: every solution once
    if rows < NK.N_SOLUTIONS[name]:
        assert handed >= 1
    else:
        assert handed == 0
    # the never-full run writes the same multiset
    ample = Raw(ctx, lb0, ub0, brancher, val, sink_rows=128)
    assert ample.run_draining(4096) == 0
    assert NK.K.multiset(ample.got_lb) == NK.K.multiset(raw.got_lb) and tuple(ample.counters.cpu().numpy()[0, :3].tolist()) == tuple(cn[:3].tolist())


# ------------------------------------------------------------------------------------------------ 3. several trees
def many_threshold(ctx):
    """The tree count from which launch_neq_dfs takes 128-thread workgroups, read from the launcher's source."""
    import torch
    with open(os.path.join(ROOT, "pcp_amd", "csrc", "pcp_api.hip")) as f:
        m = re.search(r"const bool many = n_trees >= (\d+)u \* \(uint32_t\)c->num_cu;", f.read())
    assert m
    return int(m.group(1)) * torch.cuda.get_device_properties(ctx.device).multi_processor_count


@pytest.mark.parametrize("key", sorted(BRANCHERS))
@pytest.mark.parametrize("trees", [5, 64])
def test_several_trees_through_forest_solutions(ctx, reference, trees, key):
    from pcp_amd.search_forest import forest_solutions
    brancher, val = BRANCHERS[key]
    lb0, ub0 = NK.push(ctx, "queens8")
    info = {}
    r = forest_solutions(ctx, lb0, ub0, brancher=brancher, val=val, n_trees=trees, forest="neq", sink_capacity=7, steps_per_launch=8, capacity=4, path_capacity=1, info=info)
    seeded = r["seeded_solutions"]
    print("queens8", key, trees, counts(r), "trees", r["trees"], "seeded", seeded, "drains", info.get("drains"), "steals", info.get("steals"))
    assert r["error"] == 0 and counts(r) == reference[("queens8", key)] and r["trees"] >= trees
    assert len(r["solutions_lb"]) == 92 and NK.check_boxes("queens8", r["solutions_lb"], r["solutions_ub"]) == 0
    assert (r["solution_tree"][:seeded] == -1).all() and (r["solution_tree"][seeded:] >= 0).all() and (r["solution_tree"][seeded:] < r["trees"]).all()
    assert info["drains"] >= 1
    p = ctx.last_plan()
    assert p["path"] == 1 and p["grid"] == r["trees"] and p["block"] == 256


def test_the_expansions_solutions_come_first_as_tree_minus_one(ctx, reference):
    """More trees asked for than N-queens-6's 75-node tree ever has open nodes: the expansion finds all four solutions itself."""
    from pcp_amd.search_forest import forest_solutions
    lb0, ub0 = NK.push(ctx, "queens6")
    r = forest_solutions(ctx, lb0, ub0, n_trees=64, forest="neq", sink_capacity=1, steps_per_launch=4, capacity=8)
    print("queens6 wide expansion", counts(r), "seeded", r["seeded_solutions"], r["solution_tree"].tolist())
    assert counts(r) == reference[("queens6", "split")] and NK.check_boxes("queens6", r["solutions_lb"], r["solutions_ub"]) == 0
    assert r["seeded_solutions"] == 4 and r["trees"] == 0 and (r["solution_tree"] == -1).all()
    # ... and with few trees they share the work: the expansion's come first, the trees' behind them
    r = forest_solutions(ctx, lb0, ub0, n_trees=12, forest="neq", sink_capacity=1, steps_per_launch=4, capacity=8)
    k = r["seeded_solutions"]
    print("queens6 12 trees", counts(r), "seeded", k, r["solution_tree"].tolist())
    assert counts(r) == reference[("queens6", "split")] and NK.check_boxes("queens6", r["solutions_lb"], r["solutions_ub"]) == 0
    assert (r["solution_tree"][:k] == -1).all() and (r["solution_tree"][k:] >= 0).all()


def test_the_128_thread_launch_with_most_trees_empty(ctx, reference):
    from pcp_amd.search_forest import seed_roots_interval
    lb0, ub0 = NK.push(ctx, "queens8")
    rl, ru, st, boxes = seed_roots_interval(ctx, lb0, ub0, 48, collect_solutions=True)
    k, T = int(rl.shape[0]), many_threshold(ctx)
    assert 48 <= k < T
    pad = lambda a: np.concatenate([a.cpu().numpy(), np.repeat(a[:1].cpu().numpy(), T - k, axis=0)])
    info = {}
    r = ctx.dfs_forest_neq_solutions(pad(rl), pad(ru), sink_capacity=16, steps_per_launch=16, capacity=16, sp0=[1] * k + [0] * (T - k), info=info)
    p = ctx.last_plan()
    print("queens8 at", T, "trees:", counts(r), "expansion", (st.num_nodes, st.num_solution, st.num_failed_node), "drains", info["drains"], "steals", info["steals"])
    assert p["grid"] == T and p["block"] == 128
    assert r["error"] == 0 and r["open"] == 0 and info["drains"] >= 1
    assert (r["nodes"] + st.num_nodes, r["solutions"] + st.num_solution, r["failed"] + st.num_failed_node) == reference[("queens8", "split")]
    lbs, ubs = np.concatenate([boxes[0], r["solutions_lb"]]), np.concatenate([boxes[1], r["solutions_ub"]])
    assert len(lbs) == 92 and NK.check_boxes("queens8", lbs, ubs) == 0
    assert ((r["solution_tree"] >= 0) & (r["solution_tree"] < T)).all()


# ------------------------------------------------------------------------------------------------ 4. stop_on_solution, the limit node
@pytest.mark.parametrize("key", ["split", "enum-middle"])
def test_stop_on_solution_writes_one_row_per_tree_that_found_one(ctx, key):
    from pcp_amd.search_forest import seed_roots_interval
    brancher, val = BRANCHERS[key]
    lb0, ub0 = NK.push(ctx, "queens8")
    rl, ru, _ = seed_roots_interval(ctx, lb0, ub0, 12)  # (BinarySplit's open nodes serve both: a root is a box, whatever split it further)
    raw = Raw(ctx, rl.cpu().numpy(), ru.cpu().numpy(), brancher, val, sink_rows=64, path_capacity=64)
    assert raw.call(4096, stop_on_solution=1) == 0
    cn = raw.counters.cpu().numpy()
    drawn, n = raw.drain()
    found = np.nonzero(cn[:, 1] == 1)[0]
    print("stop_on_solution", key, "trees", raw.T, "found", found.tolist(), "rows", n)
    assert set(cn[:, 1].tolist()) <= {0, 1} and (cn[:, 3] == 0).all() and len(found) >= 2
    assert drawn == n == len(found) and sorted(raw.got_tree) == found.tolist()
    stop = raw.stop.cpu().numpy()
    assert (stop[found] == 1).all() and (stop[cn[:, 1] == 0] == 0).all()
    sols = NK.brute("queens8")
    assert all(tuple(l) == tuple(u) and tuple(int(x) for x in l) in sols for l, u in zip(raw.got_lb, raw.got_ub))


@pytest.mark.parametrize("key", ["split", "enum-min"])
def test_the_limit_node_that_is_a_true_node_draws_no_ticket(ctx, key):
    brancher, val = BRANCHERS[key]
    lb0, ub0 = NK.push(ctx, "queens6")
    walk = Raw(ctx, lb0, ub0, brancher, val)
    limit = 0
    while int(walk.counters[0, 1]) == 0:  # node by node to the first True node
        assert walk.call(1) == 0
        limit += 1
        assert limit < 200
    assert int(walk.counters[0, 0]) == limit and int(walk.s_count[0]) == 1
    raw = Raw(ctx, lb0, ub0, brancher, val)
    assert raw.call(4096, node_limit=limit) == 0
    cn = raw.counters.cpu().numpy()[0]
    want = count_only(ctx, lb0, ub0, brancher, val, node_limit_per_tree=limit, steps_per_launch=64, capacity=64)
    print("limit node", key, limit, cn.tolist(), counts(want))
    assert tuple(cn[:3].tolist()) == counts(want) == (limit, 0, int(walk.counters[0, 2])) and cn[3] == 0 and int(raw.stop[0]) == 1
    assert raw.drain() == (0, 0)  # counted as a node; no ticket, no row
    # one node more and it is a solution with its row
    raw = Raw(ctx, lb0, ub0, brancher, val)
    assert raw.call(4096, node_limit=limit + 1) == 0
    assert raw.counters.cpu().numpy()[0, :2].tolist() == [limit + 1, 1] and raw.drain() == (1, 1)


# ------------------------------------------------------------------------------------------------ 5. error 6 next to the exclusion path
def test_a_full_sink_under_enumerate_leaves_the_rows_words_and_resumes_on_the_same_path(ctx):
    lb0, ub0 = NK.push(ctx, "queens6")
    whole = NC.TreeSim(6, "middle")
    whole.run()
    need = whole.max_path  # a path just sufficient: one entry less and the tree reports error 5 (test_neq_enum_forest_gpu.py)
    assert need >= 2
    raw = Raw(ctx, lb0, ub0, "enumerate", "middle", sink_rows=1, path_capacity=need)
    assert raw.call(4096) == 0
    cn = raw.counters.cpu().numpy()[0]
    sp = int(raw.sp[0])
    assert cn[3] == 6 and int(raw.stop[0]) == 1 and cn[1] == 1 and sp >= 1 and int(raw.s_count[0]) == 2
    sim = NC.TreeSim(6, "middle")
    for _ in range(int(cn[0])):
        sim.step()
    assert sim.sp == sp and sim.solutions == 1  # the node on top is the simulator's next one: not yet counted
    L, U, base, own, _ = sim.top()
    n_list = base + (own[0] != NC.NONE)
    assert int(raw.row_base[0, sp - 1]) == n_list and int(raw.row_excl[0, sp - 1, 0]) == NONE  # its list is in the path, no entry of its own
    top_l, top_u = raw.lb[0, sp - 1].cpu().numpy(), raw.ub[0, sp - 1].cpu().numpy()
    assert (top_l >= L).all() and (top_u <= U).all() and tuple(int(x) for x in top_l) in NK.brute("queens6") and (top_l == top_u).all()  # at its fixpoint: a solution
    sim.step()
    assert sim.last[3] == 1 and sim.solutions == 2  # ... and the simulator's next node is that solution
    assert raw.call(4096) == 0 and raw.counters.cpu().numpy()[0].tolist() == cn.tolist()  # stopped: another call changes nothing
    assert raw.drain() == (2, 1)  # the first solution's row and the hand-back's ticket; the idle call drew nothing
    raw.counters[0, 3] = 0
    raw.stop[0] = 0
    handed = raw.run_draining(4096)
    cn = raw.counters.cpu().numpy()[0]
    print("error 6 under Enumerate: path", need, "counters", cn.tolist(), "later hand-backs", handed)
    assert tuple(cn[:3].tolist()) == ENUM_TREE[(6, "middle")] and cn[3] == 0 and int(raw.sp[0]) == 0  # the same path sufficed: no error 5
    assert NK.check_boxes("queens6", raw.got_lb, raw.got_ub) == 0 and len(raw.got_lb) == 4


# ------------------------------------------------------------------------------------------------ 6. refusals, malformed sinks
def test_refusals_and_malformed_sinks(ctx, reference):
    import pcp_amd.engine as E
    import small_forest_cases as C
    import form_forest_cases as FC

    def counting_entry_still_counts():
        l8, u8 = NK.push(ctx, "queens8")
        r = ctx.dfs_forest(l8[None], u8[None], steps_per_launch=64, capacity=64)
        assert r["error"] == 0 and counts(r) == reference[("queens8", "split")]
        return l8, u8

    def refused(rc, code, *words):
        msg = ctx._L.pcp_last_error(ctx._h).decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    lb0, ub0 = counting_entry_still_counts()
    for brancher in ("split", "enumerate"):
        raw = Raw(ctx, lb0, ub0, brancher, capacity=16)
        assert raw.call(0) == 0 and int(raw.counters[0, 0]) == 0 and int(raw.sp[0]) == 1  # n_steps = 0: PCP_OK, nothing is launched
        # malformed sinks: PCP_ERR_ARG
        refused(raw.call(4, sink=False), -1, "null sink")
        refused(raw.call(4, sink_over={"lb": None}), -1, "lb, ub and count")
        refused(raw.call(4, sink_over={"ub": None}), -1, "lb, ub and count")
        refused(raw.call(4, sink_over={"count": None}), -1, "lb, ub and count")
        refused(raw.call(4, sink_over={"capacity": 0}), -1, "capacity")
        refused(raw.call(4, sink_over={"reserved": 1}), -1, "reserved")
        refused(raw.call(4, st=False), -1, "null state")
        refused(raw.call(4, st_over={"capacity": 1}), -1, "capacity < 2")
        if brancher == "enumerate":
            refused(raw.call(4, ex_over={"val": 2}), -1, "val")
            refused(raw.call(4, ex_over={"row_base": None}), -1, "row_base")
        # PCP_ERR_UNSUPPORTED
        sink = E.SolutionSink(8, len(lb0), raw.dev)
        ctx.solution_sink_set(sink)
        try:
            rc = raw.call(4)
            refused(rc, -5, "sink", "pcp_solution_sink_set")
        finally:
            ctx.solution_sink_set(None)
        with E.var_select_scope(ctx, "input_order"):
            refused(raw.call(4), -5, "PCP_VAR_INPUT_ORDER")
        ctx.set_option("implicit_active", 0)
        try:
            rc = raw.call(4)
        finally:
            ctx.set_option("implicit_active", 1)
        refused(rc, -5, "explicit-active")
        # nothing was launched by any of them: no ticket, no row, the tree where it was — and the same call with good arguments runs
        assert int(raw.counters[0, 0]) == 0 and int(raw.sp[0]) == 1 and int(raw.s_count[0]) == 0 and int((raw.s_lb != SENTINEL).sum()) == 0
        assert raw.run_draining(4096) == 0
        assert tuple(raw.counters.cpu().numpy()[0, :3].tolist()) == reference[("queens8", "split" if brancher == "split" else "enum-middle")]
        assert NK.check_boxes("queens8", raw.got_lb, raw.got_ub) == 0
    # a null tree pointer is allowed
    raw = Raw(ctx, lb0, ub0, capacity=16)
    assert raw.call(4096, sink_over={"tree": None}) == 0
    assert int(raw.s_count[0]) == 92 and (raw.s_tree == SENTINEL).all() and int(raw.counters[0, 1]) == 92
    # stores of other kinds
    vs, cs, _ = C.golomb(5)
    M.push_model(ctx, cs, len(vs))
    gl, gu = vs.bounds()
    refused(Raw(ctx, gl, gu, capacity=16).call(4), -5, "all-XNeqY", "pcp_dfs_forest_device_small")
    vs, cs, _ = FC.schedule("A4")
    M.push_model(ctx, cs, len(vs))
    sl, su = vs.bounds()
    refused(Raw(ctx, sl, su, capacity=16).call(4), -5, "all-XNeqY", "pcp_dfs_forest_device_form")
    props = M.lower_units([M.XNeqY(M.Identity(0), M.Identity(1))], 2)
    ctx.set_model(2, props, set_words=1)
    ctx.set_hull(0, 5)
    refused(Raw(ctx, np.zeros(2, np.int32), np.full(2, 5, np.int32), capacity=16).call(4), -1, "interval-mode")
    # ... and the counting entries, with nothing attached, give the counts they gave
    counting_entry_still_counts()
    r = ctx.dfs_forest_enum(lb0[None], ub0[None], forest="neq", steps_per_launch=64, capacity=64)
    assert counts(r) == ENUM_TREE[(8, "middle")]
