"""Enumerate in the formula-store forest on the device (pcp_dfs_forest_device_form_enum; formdfs_kernel<BNB, true, SINK>, pcp_formdfs.hip):
one tree against FormTreeSim's rows, row words, path and counters at every launch seam; complete trees against the host specification;
the sweep's lane stride and rounds; tree indexing; the errors 1, 5 and 2 and the StopNode limit node; branch and bound; the solution sink;
start windows below zero; growth and refill; the contract; the dispatch by store and BinarySplit untouched.  The reference of every
comparison is the oracle-backed host specification (test_form_enum_forest_cpu.py checks FormTreeSim against it), never the kernel."""
import ctypes as C_

import numpy as np
import pytest

import form_enum_forest_cases as EC
import form_excl_cases as X
import form_forest_cases as FC
from pcp_amd import model as M
from test_form_enum_forest_cpu import NAME, spec
from test_form_excl_cpu import reference, reference_bnb_enum

pytestmark = pytest.mark.gpu

NONE = -1  # row_excl[r].var == 0xFFFFFFFF as int32


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


def counts(r):
    return r["nodes"], r["solutions"], r["failed"]


class Raw:
    """The buffers of n trees and the C entry itself, one call per launch.  ``lists``: the exclusions each root arrives with."""

    def __init__(self, ctx, lbs, ubs, capacity=64, path_capacity=160, val="middle", objective=None, lists=None):
        import torch
        import pcp_amd.engine as E
        self.E, self.ctx, self.torch = E, ctx, torch
        self.dev = dev = torch.device("cuda", ctx.device)
        lbs, ubs = np.atleast_2d(lbs).astype(np.int32), np.atleast_2d(ubs).astype(np.int32)
        T, V = lbs.shape
        self.T, self.V, self.cap = T, V, capacity
        z = self.z
        self.lb, self.ub = z(T, capacity, V), z(T, capacity, V)
        self.lb[:, 0], self.ub[:, 0] = torch.from_numpy(lbs).to(dev), torch.from_numpy(ubs).to(dev)
        self.sp, self.stop = torch.ones(T, dtype=torch.int32, device=dev), z(T)
        self.status, self.counters = z(T, capacity, dt=torch.uint8), z(T, 5, dt=torch.int64)
        self.row_base, self.row_excl = z(T, capacity), z(T, capacity, 2)
        self.row_excl[:, :, 0] = NONE
        self.val = E.VAL_MODES[val]
        self.path = None
        self.set_path(path_capacity)
        for t, e in enumerate(lists or []):
            if len(e):
                self.path[t, :len(e)] = torch.tensor(e, dtype=torch.int32, device=dev)
            self.row_base[t, 0] = len(e)
        self.obj = None
        if objective is not None:
            var, mode = objective
            self.best = torch.full((1,), E.no_incumbent(mode), dtype=torch.int32, device=dev)
            self.tree_best = torch.full((T,), E.no_incumbent(mode), dtype=torch.int32, device=dev)
            self.tree_row = z(T, V)
            self.obj = E.ForestObjective(var, E.OBJ_MODES[mode], self.best.data_ptr(), self.tree_best.data_ptr(), self.tree_row.data_ptr())

    def z(self, *s, dt=None):
        return self.torch.zeros(s, dtype=dt or self.torch.int32, device=self.dev)

    def set_path(self, path_capacity):
        old = self.path
        self.path = self.z(self.T, max(path_capacity, 1), 2)
        if old is not None:
            k = min(old.shape[1], self.path.shape[1])
            self.path[:, :k] = old[:, :k]
        self.path_capacity = path_capacity

    def set_capacity(self, capacity):
        """A larger stack: the rows and their words move along."""
        k = self.cap
        for name in ("lb", "ub", "status", "row_base", "row_excl"):
            old = getattr(self, name)
            new = self.torch.zeros((self.T, capacity) + tuple(old.shape[2:]), dtype=old.dtype, device=self.dev)
            new[:, :k] = old
            setattr(self, name, new)
        self.cap = capacity

    def resume(self):
        self.counters[:, 3] = 0
        self.stop.zero_()

    def call(self, n_steps, stop_on_solution=0, node_limit=0, ex=True, st_over=None, ex_over=None):
        E = self.E
        st = E.DfsState(self.lb.data_ptr(), self.ub.data_ptr(), self.cap, self.sp.data_ptr(), self.stop.data_ptr(), self.status.data_ptr(), self.counters.data_ptr(),
                        None, None)
        x = E.ForestExcl(self.path.data_ptr() if self.path_capacity else None, self.row_base.data_ptr(), self.row_excl.data_ptr(), self.path_capacity, self.val)
        for k, v in (ex_over or {}).items():
            setattr(x, k, v)
        for k, v in (st_over or {}).items():
            setattr(st, k, v)
        rc = getattr(self.ctx._L, NAME)(self.ctx._h, C_.byref(st), self.T, C_.byref(x) if ex else None,
                                        C_.byref(self.obj) if self.obj is not None else None, n_steps, stop_on_solution, node_limit, None)
        self.torch.cuda.synchronize()
        return rc

    def live(self):
        return bool(((self.sp > 0) & (self.stop == 0)).any())

    def run(self, n_steps, max_launches=1 << 20, **kw):
        for _ in range(max_launches):
            assert self.call(n_steps, **kw) == 0
            if not self.live():
                break
        return self.counters.cpu().numpy()

    def same_as(self, sim, t=0):
        """Tree t is what FormTreeSim holds: sp, the rows [0, sp) with their two words, path[0 .. row_base[top]) and the counters."""
        sp = int(self.sp[t])
        assert sp == sim.sp, (sp, sim.sp, sim.nodes)
        assert tuple(self.counters[t, :3].cpu().tolist()) == (sim.nodes, sim.solutions, sim.failed), sim.nodes
        if not sp:
            return
        lb, ub = self.lb[t, :sp].cpu().numpy(), self.ub[t, :sp].cpu().numpy()
        base, own = self.row_base[t, :sp].cpu().numpy(), self.row_excl[t, :sp].cpu().numpy()
        for r in range(sp):
            assert np.array_equal(lb[r], sim.rows[r][0]) and np.array_equal(ub[r], sim.rows[r][1]), (sim.nodes, r)
            assert int(base[r]) == sim.row_base[r], (sim.nodes, r)
            e = sim.row_excl[r]
            assert (own[r, 0] == NONE) if e is None else (tuple(own[r].tolist()) == e), (sim.nodes, r)
        top = sim.row_base[sp - 1]
        assert [tuple(p) for p in self.path[t, :top].cpu().numpy().tolist()] == sim.path[:top], sim.nodes


def plan_is_form(ctx, grid):
    p = ctx.last_plan()
    return p["path"] == 3 and p["grid"] == grid and p["block"] == 256


# ------------------------------------------------------------------------------------------------ 1. one tree at launch seams
@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("steps", [1, 2, 3, 7, 0])
def test_one_tree_is_the_specification_at_launch_seams(ctx, steps, val):
    key = "search:A4"
    X.push(ctx, key)
    lb0, ub0 = EC.root_of(key)
    whole = EC.tree(key, val)
    steps = steps or whole.nodes + 7  # 0: the whole tree in one launch
    raw, sim = Raw(ctx, lb0, ub0, val=val), EC.FormTreeSim(key, val)
    while sim.sp:
        assert raw.call(steps) == 0
        for _ in range(steps):
            if sim.sp:
                sim.step()
        raw.same_as(sim)
    assert plan_is_form(ctx, 1) and int(raw.counters[0, 3]) == 0
    assert (sim.nodes, sim.solutions, sim.failed) == (whole.nodes, whole.solutions, whole.failed) == EC.counts(spec("A4", val)[0])


# ------------------------------------------------------------------------------------------------ 2. complete trees
@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("name", EC.SEARCH_NAMES)
def test_complete_trees_are_the_host_specifications(ctx, name, val):
    """(The five-task model without an objective: its first WALK_LIMIT nodes under StopNode — form_enum_forest_cases.py says why.)"""
    key = "search:" + name
    X.push(ctx, key)
    lb0, ub0 = EC.root_of(key)
    want = EC.counts(spec(name, val)[0])
    limit = EC.WALK_LIMIT.get(name, 0)
    info = {}
    r = ctx.dfs_forest_enum(lb0[None], ub0[None], val=val, steps_per_launch=512, capacity=64, node_limit_per_tree=limit, info=info)
    print(name, val, counts(r), want, "path", info["path_capacity"])
    assert plan_is_form(ctx, 1) and r["error"] == 0 and (r["open"] > 0) == bool(limit) and counts(r) == want


# ------------------------------------------------------------------------------------------------ 3. the sweep's lane stride and rounds
def test_lists_around_the_wavefront_width_and_the_chain(ctx):
    """Roots of "wide" with lists of 63, 64, 65 and 130 entries and the chain cases (70 values that fall one a round), one step each in one
    launch: the node left — the right child in row 0, the left child on top — is the judge's."""
    X.push(ctx, "wide")
    roots = EC.sweep_roots()
    raw = Raw(ctx, np.stack([r[0] for r in roots]), np.stack([r[1] for r in roots]), capacity=4, lists=[r[2] for r in roots])
    ctx.stats_reset()
    assert raw.call(1) == 0
    stats = ctx.stats_read()
    assert stats["waves"] >= X.CHAIN  # the chain's node alone took that many rounds
    for t, (lb0, ub0, ex) in enumerate(roots):
        sim = EC.FormTreeSim("wide", "middle", root=(lb0, ub0), root_excl=ex)
        sim.step()
        raw.same_as(sim, t)


def test_more_than_64_slots_and_units_under_a_path(ctx):
    """The six-task store (a lane runs two units, two slots) under MiddleVal, whose path is not empty: 240 nodes, compared at every seam."""
    V = X.push(ctx, "six")
    assert V > 64 and ctx.n_units > 64
    lb0, ub0 = EC.root_of("six")
    ex = [(0, 3), (2, 4)]
    raw, sim = Raw(ctx, lb0, ub0, lists=[ex]), EC.FormTreeSim("six", "middle", root_excl=ex)
    for _ in range(6):
        assert raw.call(40) == 0
        for _ in range(40):
            sim.step()
        raw.same_as(sim)
    assert sim.max_path > len(ex) and sim.nodes == 240


# ------------------------------------------------------------------------------------------------ 4. tree indexing and LDS slices
def open_rows(key, val, want):
    """The `want` topmost open nodes of the tree, as roots of their own — [(lb, ub, list)] — at the first moment at which it holds that many
    and one of them carries a list."""
    sim = EC.FormTreeSim(key, val)
    rows = []
    while not (len(rows) == want and any(len(r[2]) for r in rows)):
        sim.step()
        assert sim.sp, "the tree never holds that many open nodes with a list"
        rows = [(sim.rows[r][0], sim.rows[r][1], sim.path[:sim.row_base[r]] + ([sim.row_excl[r]] if sim.row_excl[r] is not None else []))
                for r in range(max(sim.sp - want, 0), sim.sp)]
    return rows


@pytest.mark.parametrize("T", [3, 5])
def test_a_partial_workgroup_and_an_idle_tree(ctx, T):
    key = "search:A4"
    X.push(ctx, key)
    roots = open_rows(key, "middle", T)
    idle = 0
    raw = Raw(ctx, np.stack([r[0] for r in roots]), np.stack([r[1] for r in roots]), capacity=32, lists=[r[2] for r in roots])
    raw.sp[idle] = 0
    raw.lb[idle], raw.ub[idle] = -77, -77
    cn = raw.run(1 << 16)
    assert plan_is_form(ctx, -(-T // 4)) and (raw.sp == 0).all() and (cn[:, 3] == 0).all()
    assert cn[idle].tolist() == [0, 0, 0, 0, 0] and (raw.lb[idle] == -77).all() and (raw.ub[idle] == -77).all()
    for t, (lb0, ub0, ex) in enumerate(roots):
        if t != idle:
            assert tuple(cn[t, :3].tolist()) == EC.FormTreeSim(key, "middle", root=(lb0, ub0), root_excl=ex).run(), t


# ------------------------------------------------------------------------------------------------ 5. errors
def test_error_1_keeps_the_node_propagated_and_uncounted(ctx):
    key = "search:A4"
    X.push(ctx, key)
    lb0, ub0 = EC.root_of(key)
    whole = EC.tree(key, "middle")
    raw, sim = Raw(ctx, lb0, ub0, capacity=2), EC.FormTreeSim(key, "middle")
    assert raw.call(64) == 0
    sim.step()                                   # the root: counted, two rows
    L, U, base, own, path = sim.top()            # the left child: run, found Unknown with the stack full, kept
    st, lb, ub = EC.judge(key, L, U, path)
    assert st == 2
    assert int(raw.sp[0]) == 2 and int(raw.stop[0]) == 1 and raw.counters[0, :4].cpu().tolist() == [1, 0, 0, 1]
    assert np.array_equal(raw.lb[0, 1].cpu().numpy(), lb) and np.array_equal(raw.ub[0, 1].cpu().numpy(), ub)
    assert int(raw.row_base[0, 1]) == base and int(raw.row_excl[0, 1, 0]) == NONE
    raw.set_capacity(64)
    raw.resume()
    cn = raw.run(512)[0]
    assert cn[3] == 0 and int(raw.sp[0]) == 0 and tuple(cn[:3].tolist()) == (whole.nodes, whole.solutions, whole.failed)


@pytest.mark.parametrize("inherited", [0, 1])
def test_error_5_leaves_the_row_alone(ctx, inherited):
    """path_capacity = 0, and = exactly row_base with one inherited entry: a popped row with an entry of its own has nowhere to put it."""
    key = "search:A4"
    X.push(ctx, key)
    lb0, ub0 = EC.root_of(key)
    first, own = [(0, 2)][:inherited], (1, 3)
    assert lb0[1] < 3 < ub0[1]
    raw = Raw(ctx, lb0, ub0, path_capacity=inherited, lists=[first])
    raw.row_excl[0, 0, 0], raw.row_excl[0, 0, 1] = own
    assert raw.call(64) == 0
    assert int(raw.sp[0]) == 1 and int(raw.stop[0]) == 1 and raw.counters[0, :4].cpu().tolist() == [0, 0, 0, 5]
    assert np.array_equal(raw.lb[0, 0].cpu().numpy(), lb0) and np.array_equal(raw.ub[0, 0].cpu().numpy(), ub0)
    assert raw.row_excl[0, 0].cpu().tolist() == list(own) and int(raw.row_base[0, 0]) == inherited
    raw.set_path(64)
    raw.resume()
    cn = raw.run(512)[0]
    assert cn[3] == 0 and int(raw.sp[0]) == 0 and tuple(cn[:3].tolist()) == EC.FormTreeSim(key, "middle", root_excl=first + [own]).run()


@pytest.mark.parametrize("where", ["row", "path", "base"])
def test_a_malformed_entry_stops_its_tree_alone(ctx, where):
    import pcp_amd.engine as E
    key = "search:A4"
    V = X.push(ctx, key)
    lb0, ub0 = EC.root_of(key)
    whole = EC.tree(key, "middle")
    ctx.stats_read()
    raw = Raw(ctx, np.stack([lb0] * 4), np.stack([ub0] * 4), path_capacity=32)
    if where == "row":
        raw.row_excl[0, 0, 0], raw.row_excl[0, 0, 1] = V, 3
    elif where == "path":
        raw.path[0, 0, 0], raw.path[0, 0, 1] = V, 3
        raw.row_base[0, 0] = 1
    else:
        raw.row_base[0, 0] = 33
    cn = raw.run(1 << 16)
    print("malformed", where, cn.tolist())
    assert cn[0, :4].tolist() == [1, 0, 0, 2] and int(raw.stop[0]) == 1 and int(raw.sp[0]) == 0  # counted and popped, stopped alone
    for t in (1, 2, 3):
        assert tuple(cn[t, :3].tolist()) == (whole.nodes, whole.solutions, whole.failed) and cn[t, 3] == 0 and int(raw.sp[t]) == 0
    with pytest.raises(E.PcpError) as e:  # the sticky violation word; reading it reports and clears it
        ctx.stats_read()
    assert e.value.code == -2
    ctx.stats_read()


@pytest.mark.parametrize("val", ["middle", "min"])
def test_the_limit_node_is_a_node_and_nothing_else(ctx, val):
    key = "search:A4"
    X.push(ctx, key)
    lb0, ub0 = EC.root_of(key)
    sim = EC.FormTreeSim(key, val)
    while not sim.solutions:
        before = (sim.nodes, sim.solutions, sim.failed)
        sim.step()
    k = sim.nodes  # the first solution is node k
    raw = Raw(ctx, lb0, ub0, val=val)
    cn = raw.run(5, node_limit=k)[0]
    assert cn[:4].tolist() == [k, 0, before[2], 0] and int(raw.stop[0]) == 1
    raw = Raw(ctx, lb0, ub0, val=val)
    cn = raw.run(5, node_limit=k + 1)[0]
    assert cn[0] == k + 1 and cn[1] == 1


# ------------------------------------------------------------------------------------------------ 6. branch and bound
@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("mode", ["min", "max"])
def test_one_tree_of_branch_and_bound_is_the_reference(ctx, mode, val):
    key = "search:C4mk"
    X.push(ctx, key)
    lb0, ub0 = EC.root_of(key)
    mk = X.store(key)[2]
    ref = reference_bnb_enum(key, lb0, ub0, mk, mode, val)
    assert 0 < ref["nodes"] <= X.TREE_CEILING and ref["solutions"] >= 1
    raw = Raw(ctx, lb0, ub0, objective=(mk, mode), val=val)
    seq, solved = [], 0
    while raw.live():
        assert raw.call(1) == 0
        if int(raw.counters[0, 1]) > solved:
            solved = int(raw.counters[0, 1])
            seq.append(int(raw.tree_best[0]))
    cn = raw.counters[0].cpu().tolist()
    print("C4mk", mode, val, cn, seq)
    assert cn[:4] == [ref["nodes"], ref["solutions"], ref["failed"], 0] and seq == ref["incumbents"]
    assert int(raw.best[0]) == ref["best"] and np.array_equal(raw.tree_row[0].cpu().numpy(), ref["row"])
    r = ctx.dfs_forest_enum(lb0[None], ub0[None], val=val, objective=(mk, mode), steps_per_launch=64, capacity=64)  # ... and in launches of 64
    assert counts(r) == (ref["nodes"], ref["solutions"], ref["failed"]) and r["best"] == ref["best"] and np.array_equal(r["best_solution"], ref["row"])


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("trees", [1, 3, 64])
def test_a_forest_of_branch_and_bound_finds_the_optimum(ctx, trees, val):
    from pcp_amd.search_forest import forest_enumerate
    key = "search:D5mk"
    X.push(ctx, key)
    lb0, ub0 = EC.root_of(key)
    mk = X.store(key)[2]
    best = reference("D5mk", val)["best"]
    if trees == 1:
        r = ctx.dfs_forest_enum(lb0[None], ub0[None], val=val, objective=(mk, "min"), steps_per_launch=128, capacity=64)
    else:
        r = forest_enumerate(ctx, lb0, ub0, val=val, objective=(mk, "min"), n_trees=trees, steps_per_launch=32, capacity=64)
    print("D5mk", trees, val, counts(r), r["best"])
    assert ctx.last_plan()["path"] == 3
    assert r["error"] == 0 and r["open"] == 0 and r["best"] == best and r["nodes"] > 0
    row = np.asarray(r["best_solution"], np.int32)
    assert int(row[mk]) == best and FC.is_schedule("D5mk", row)


# ------------------------------------------------------------------------------------------------ 7. the solution sink
@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("trees", [1, 5])
def test_every_schedule_once_through_the_sink(ctx, trees, val):
    from pcp_amd.search_forest import forest_enumerate
    key = "search:A4"
    X.push(ctx, key)
    lb0, ub0 = EC.root_of(key)
    info = {}
    r = forest_enumerate(ctx, lb0, ub0, val=val, n_trees=trees, steps_per_launch=64, capacity=64, collect_solutions=True, sink_capacity=37, info=info)
    want = EC.counts(spec("A4", val)[0])
    print("A4 sink", trees, val, counts(r), "drains", info.get("drains"), "seeded", r["seeded_solutions"])
    assert r["error"] == 0 and counts(r) == want and len(r["solutions_lb"]) == r["solutions"]
    pts, total = X.covered(4, list(zip(r["solutions_lb"], r["solutions_ub"])))
    assert pts == set(X.all_schedules("A4")) and total == len(pts)
    if trees == 1:
        assert info["drains"] > 0


@pytest.mark.parametrize("val", ["middle", "min"])
def test_the_raw_entry_hands_back_at_a_full_sink(ctx, val):
    import torch
    import pcp_amd.engine as E
    key = "search:A4"
    X.push(ctx, key)
    lb0, ub0 = EC.root_of(key)
    whole = EC.tree(key, val)
    count = whole.solutions
    want = sorted(tuple(l.tolist()) + tuple(u.tolist()) for l, u in whole.boxes)
    for cap in (1, 2, count - 1, count):
        raw = Raw(ctx, lb0, ub0, val=val)
        s_lb, s_ub, s_tree, s_count = raw.z(cap, raw.V), raw.z(cap, raw.V), raw.z(cap), raw.z(1)
        sink = E.PcpSolutionSink(s_lb.data_ptr(), s_ub.data_ptr(), s_tree.data_ptr(), s_count.data_ptr(), cap, 0)
        assert ctx._L.pcp_solution_sink_set(ctx._h, C_.byref(sink)) == 0
        got, hand_backs = [], 0
        try:
            for _ in range(count + 8):
                assert raw.call(1 << 14) == 0
                n = min(int(s_count[0]), cap)
                got += [tuple(a) + tuple(b) for a, b in zip(s_lb[:n].cpu().tolist(), s_ub[:n].cpu().tolist())]
                s_count.zero_()
                if int(raw.counters[0, 3]) == 6:
                    hand_backs += 1
                    assert int(raw.stop[0]) == 1 and int(raw.row_excl[0, int(raw.sp[0]) - 1, 0]) == NONE
                    raw.resume()
                if not raw.live():
                    break
        finally:
            assert ctx._L.pcp_solution_sink_set(ctx._h, None) == 0
        cn = raw.counters[0].cpu().tolist()
        assert cn[:4] == [whole.nodes, whole.solutions, whole.failed, 0] and int(raw.sp[0]) == 0, cap
        assert sorted(got) == want and (hand_backs > 0) == (cap < count), cap  # no row lost, none doubled
        if cap == 1:  # with an objective a sink is refused and nothing is launched
            assert ctx._L.pcp_solution_sink_set(ctx._h, C_.byref(sink)) == 0
            try:
                rb = Raw(ctx, lb0, ub0, val=val, objective=(3, "max"))
                assert rb.call(8) == -5 and "sink" in ctx._L.pcp_last_error(ctx._h).decode()
                assert int(rb.counters[0, 0]) == 0 and int(rb.sp[0]) == 1
            finally:
                assert ctx._L.pcp_solution_sink_set(ctx._h, None) == 0


# ------------------------------------------------------------------------------------------------ 8. start windows below zero
@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("shift", [-4, -2])
def test_windows_below_and_across_zero(ctx, shift, val):
    """MiddleVal truncates toward zero: the tree of a shifted window is not the shifted tree."""
    vs, cs, _, lb0, ub0 = EC.shifted("A4", shift)
    M.push_model(ctx, cs, len(vs))
    assert lb0[0] < 0 < ub0[0]
    want = EC.FormTreeSim(("A4", shift), val)
    want.run()
    r = ctx.dfs_forest_enum(lb0[None], ub0[None], val=val, steps_per_launch=256, capacity=64)
    print("A4 shifted", shift, val, counts(r))
    assert r["error"] == 0 and r["open"] == 0 and counts(r) == (want.nodes, want.solutions, want.failed)
    if val == "middle":
        assert want.max_path >= 1


# ------------------------------------------------------------------------------------------------ 9. growth and refill
@pytest.mark.parametrize("name", ["C4mk", "D5mk"])
def test_growth_and_refill(ctx, name):
    """Eight trees, two-row stacks, a one-entry path, rebalancing on: stacks and paths grow, finished trees steal with the lists moving
    along, and the expansion plus the trees are the complete tree's counters — C4mk's from a fresh search of the host specification, eight
    nodes a launch; D5mk's (284 679 nodes) from form_enum_forest_cases.D5MK_COMPLETE, 256 nodes a launch."""
    from pcp_amd.search_forest import forest_enumerate
    key = "search:" + name
    X.push(ctx, key)
    lb0, ub0 = EC.root_of(key)
    want = EC.D5MK_COMPLETE["middle"] if name == "D5mk" else EC.counts(spec(name, "middle")[0])
    info = {}
    r = forest_enumerate(ctx, lb0, ub0, val="middle", n_trees=8, steps_per_launch=256 if name == "D5mk" else 8, capacity=2, path_capacity=1, info=info)
    print("growth and refill", name, counts(r), {k: info.get(k) for k in ("grown", "path_grown", "steals", "capacity", "path_capacity", "launches")})
    assert r["error"] == 0 and r["trees"] >= 8 and counts(r) == want
    assert info["grown"] > 0 and info["path_grown"] > 0 and info["steals"] > 0


# ------------------------------------------------------------------------------------------------ 10. the contract
def test_contract(ctx):
    import pcp_amd.engine as E
    key = "search:C4mk"
    X.push(ctx, key)
    lb0, ub0 = EC.root_of(key)
    mk = X.store(key)[2]
    err = lambda: ctx._L.pcp_last_error(ctx._h).decode()
    raw = Raw(ctx, lb0, ub0, capacity=16, objective=(mk, "min"))
    assert raw.call(0) == 0 and int(raw.counters[0, 0]) == 0 and int(raw.sp[0]) == 1  # n_steps = 0: PCP_OK, nothing is launched
    assert raw.call(0, ex=False) == -1 and NAME in err()
    assert raw.call(0, ex_over={"val": 2}) == -1 and NAME in err()
    assert raw.call(0, ex_over={"row_base": None}) == -1 and raw.call(0, ex_over={"row_excl": None}) == -1
    assert raw.call(0, ex_over={"path": None}) == -1                       # path_capacity > 0 and no path
    assert raw.call(0, ex_over={"path": None, "path_capacity": 0}) == 0
    assert raw.call(0, st_over={"capacity": 1}) == -1 and raw.call(0, st_over={"lb": None}) == -1 and raw.call(0, st_over={"counters": None}) == -1
    raw.T = 0
    assert raw.call(0) == -1
    raw.T = 1
    for bad in (E.ForestObjective(len(lb0), 0, raw.best.data_ptr(), raw.tree_best.data_ptr(), None), E.ForestObjective(mk, 2, raw.best.data_ptr(), raw.tree_best.data_ptr(), None),
                E.ForestObjective(mk, 0, None, raw.tree_best.data_ptr(), None), E.ForestObjective(mk, 0, raw.best.data_ptr(), None, None)):
        raw.obj = bad
        assert raw.call(0) == -1
    raw.obj = None
    assert raw.call(0) == 0
    assert getattr(ctx._L, NAME)(ctx._h, None, 1, None, None, 0, 0, 0, None) == -1  # a null state
    # stop_on_solution without an objective stops at the first solution; with one it is ignored
    one = ctx.dfs_forest_enum(lb0[None], ub0[None], stop_on_solution=True, want_solution=True, steps_per_launch=64, capacity=64)
    assert one["solutions"] == 1 and FC.is_schedule("C4mk", one["first_solutions"][0])
    rb = Raw(ctx, lb0, ub0, objective=(mk, "min"))
    rb.run(64, stop_on_solution=1)
    ref = reference("C4mk", "middle")
    assert tuple(rb.counters[0, :3].cpu().tolist()) == (ref["nodes"], ref["solutions"], ref["failed"]) and int(rb.best[0]) == ref["best"]
    # a store without formula units: the small-store entry is named
    import small_forest_cases as C
    vs, cs, _ = C.golomb(5)
    M.push_model(ctx, cs, len(vs))
    l0, u0 = (np.ascontiguousarray(a, np.int32) for a in vs.bounds())
    assert Raw(ctx, l0, u0).call(0) == -5 and "pcp_dfs_forest_device_small_enum" in err() and NAME in err()
    # a node beyond one CU's LDS (8 bytes per slot)
    vs, cs = M.VStore(), M.CStore()
    starts = [vs.alloc((0, 5)) for _ in range(2)]
    cap = vs.alloc((FC.CAPACITY, FC.CAPACITY))
    M.Cumulative(starts, [M.Constant(2), M.Constant(2)], [M.Constant(2), M.Constant(2)], cap).join(vs, cs)
    for _ in range(21000):
        vs.alloc((0, 1))
    M.push_model(ctx, cs, len(vs))
    l0, u0 = (np.ascontiguousarray(a, np.int32) for a in vs.bounds())
    assert Raw(ctx, l0, u0, capacity=2, path_capacity=1).call(0) == -5 and "LDS" in err() and NAME in err()
    # a set-mode model
    props = M.lower_units([M.XNeqY(M.Identity(0), M.Identity(1)), M.XLessY(M.Identity(2), M.Identity(3))], 4)
    ctx.set_model(4, props, set_words=1)
    ctx.set_hull(0, 5)
    assert Raw(ctx, np.zeros((2, 4), np.int32), np.full((2, 4), 5, np.int32), capacity=16).call(0) == -1 and NAME in err()


# ------------------------------------------------------------------------------------------------ 11. dispatch, and no change elsewhere
def test_a_store_without_formula_units_goes_to_the_small_forest(ctx):
    from pcp_amd.search_forest import forest_enumerate, forest_search
    import small_forest_cases as C
    vs, cs, var = C.golomb(5)
    M.push_model(ctx, cs, len(vs))
    lb0, ub0 = (np.ascontiguousarray(a, np.int32) for a in vs.bounds())
    assert not ctx.has_formulas
    for val in ("middle", "min"):
        a = ctx.dfs_forest_enum(lb0[None], ub0[None], val=val, steps_per_launch=64, capacity=64)
        assert ctx.last_plan()["path"] == 4
        b = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=64, capacity=64, small=True, brancher="enumerate", val=val)
        assert a.keys() == b.keys() and counts(a) == counts(b) and np.array_equal(a["per_tree"], b["per_tree"]) and a["launches"] == b["launches"]
        a = forest_enumerate(ctx, lb0, ub0, val=val, n_trees=5, steps_per_launch=64, capacity=64)
        b = forest_search(ctx, lb0, ub0, n_trees=5, steps_per_launch=64, capacity=64, small=True, brancher="enumerate", val=val)
        assert a.keys() == b.keys() and counts(a) == counts(b) and a["trees"] == b["trees"]
    a = ctx.dfs_forest_enum(lb0[None], ub0[None], objective=(var, "min"), steps_per_launch=64, capacity=64)
    b = ctx.dfs_forest_bnb(lb0[None], ub0[None], (var, "min"), steps_per_launch=64, capacity=64, small=True, brancher="enumerate")
    assert counts(a) == counts(b) and a["best"] == b["best"] == C.OPTIMUM[5]


def test_binary_split_in_the_formula_forest_is_untouched(ctx):
    """dfs_forest(formulas=True) and dfs_forest_bnb on C4mk against the oracle's search and the host specification, as before."""
    from pcp_amd import search as S
    vs, cs, mk = FC.schedule("C4mk")
    M.push_model(ctx, cs, len(vs))
    lb0, ub0 = vs.bounds()
    want = FC.counts(FC.oracle_model(vs, cs).search(lb0, ub0, all_solutions=True)[0])
    r = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=64, capacity=64, formulas=True)
    assert plan_is_form(ctx, 1) and r["error"] == 0 and FC.counts(r) == want
    host = S.dfs(FC.FormulaOracleCtx(vs, cs), lb0, ub0, objective=(mk, "min"), batch=1)
    b = ctx.dfs_forest_bnb(lb0[None], ub0[None], (mk, "min"), steps_per_launch=64, capacity=64)
    assert b["error"] == 0 and FC.counts(b) == FC.counts(host) and b["best"] == host.best
