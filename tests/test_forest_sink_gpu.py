"""The solution sink of the Interval forests on the device (pcp_solution_sink_set; formdfs_kernel<false, true>, smalldfs_kernel<false, ENUM, true>):
every solution of the formula-store and of the small-store forest, under BinarySplit and Enumerate, as (lb, ub) boxes checked against a
brute-force enumeration (forest_sink_cases.py; test_forest_sink_cpu.py pins it); the hand-back protocol of a full sink at capacities 1, 2
and one short of the count; the raw entry at a seam; the StopNode limit node; stop_on_solution; the refusals of the C ABI; expansion plus
forest."""
import ctypes as C_
import functools

import numpy as np
import pytest

import forest_sink_cases as K
from pcp_amd import model as M
from pcp_amd import search as S

pytestmark = pytest.mark.gpu

# (model, kind of forest, brancher, val)
CONFIGS = [("sched3", "form", "split", "middle")] + [(m, "small", b, v) for m in ("queens6", "queens8", "golomb4")
                                                      for b, v in (("split", "middle"), ("enumerate", "middle"), ("enumerate", "min"))]
IDS = ["-".join(c) for c in CONFIGS]
LIGHT = [c for c in CONFIGS if c[0] != "queens8"]
LIGHT_IDS = ["-".join(c) for c in LIGHT]


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


def push(ctx, name):
    vs, cs = K.build(name)
    M.push_model(ctx, cs, len(vs))
    return K.root(name)


def forest_kw(kind, brancher, val):
    kw = dict(formulas=True) if kind == "form" else dict(small=True)
    if brancher == "enumerate":
        kw.update(brancher=brancher, val=val)
    return kw


def counts(r):
    return r["nodes"], r["solutions"], r["failed"]


_HOST = {}


def host_rows(ctx, cfg):
    """The lower-bound rows of the host-stepped search on this context (the model is pushed), once per configuration."""
    if cfg not in _HOST:
        name, kind, brancher, val = cfg
        lb0, ub0 = K.root(name)
        st = S.dfs(ctx, lb0, ub0, all_solutions=True) if brancher == "split" else S.dfs_enumerate(ctx, lb0, ub0, all_solutions=True, val=val)
        _HOST[cfg] = K.multiset(st.solutions)
    return _HOST[cfg]


_PLAIN = {}


def plain(ctx, cfg, trees, steps):
    """forest_search without a sink (the model is pushed), once per shape: what the counters with a sink must equal."""
    from pcp_amd.search_forest import forest_search
    key = (cfg, trees, steps)
    if key not in _PLAIN:
        name, kind, brancher, val = cfg
        r = forest_search(ctx, *K.root(name), n_trees=trees, steps_per_launch=steps, capacity=64, **forest_kw(kind, brancher, val))
        assert r["error"] == 0 and "solutions_lb" not in r
        _PLAIN[key] = (counts(r), r["trees"])
    return _PLAIN[key]


def check_set(ctx, cfg, r):
    name = cfg[0]
    lbs, ubs = r["solutions_lb"], r["solutions_ub"]
    assert lbs.dtype == ubs.dtype == np.int32 and lbs.shape == ubs.shape == (r["solutions"], len(K.root(name)[0]))
    assert len(r["solution_tree"]) == r["solutions"]
    proper = K.check_boxes(name, lbs, ubs)
    assert K.multiset(lbs) == host_rows(ctx, cfg)
    return proper


# ------------------------------------------------------------------------------------------------ 1. a sink that never fills
@pytest.mark.parametrize("steps", [1, 3, 256])
@pytest.mark.parametrize("trees", [1, 4, 64])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_every_solution_with_room_to_spare(ctx, cfg, trees, steps):
    from pcp_amd.search_forest import forest_search
    name, kind, brancher, val = cfg
    lb0, ub0 = push(ctx, name)
    info = {}
    r = forest_search(ctx, lb0, ub0, n_trees=trees, steps_per_launch=steps, capacity=64, collect_solutions=True, sink_capacity=4096, info=info,
                      **forest_kw(kind, brancher, val))
    want, n_roots = plain(ctx, cfg, trees, steps)
    print(name, kind, brancher, val, trees, steps, counts(r), "trees", r["trees"], "seeded", r["seeded_solutions"], "drains", info.get("drains"))
    assert r["error"] == 0 and counts(r) == want and r["trees"] == n_roots
    assert info.get("drains", 0) == 0
    proper = check_set(ctx, cfg, r)
    if name == "sched3":
        assert proper == 3 and r["solutions"] == 21  # three True nodes are boxes of two schedules: 24 in all
    else:
        assert proper == 0 and r["solutions"] == K.N_SOLUTIONS[name]
    tree = r["solution_tree"]
    assert ((tree >= -1) & (tree < max(r["trees"], 1))).all() and (tree[:r["seeded_solutions"]] == -1).all() and (tree[r["seeded_solutions"]:] >= 0).all()


def test_without_collect_solutions_the_result_keeps_its_keys(ctx):
    lb0, ub0 = push(ctx, "queens6")
    r = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=64, capacity=64, small=True)
    assert sorted(r) == sorted(["nodes", "solutions", "failed", "error", "open", "launches", "per_tree", "trees", "steals", "first_solutions"])
    assert counts(r) == K.SPLIT_TREE["queens6"][:3]


# ------------------------------------------------------------------------------------------------ 2. a sink that fills
@pytest.mark.parametrize("steps", [3, 256])
@pytest.mark.parametrize("trees", [1, 4])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_hand_backs_lose_nothing_and_count_nothing_twice(ctx, cfg, trees, steps):
    from pcp_amd.search_forest import forest_search
    name, kind, brancher, val = cfg
    lb0, ub0 = push(ctx, name)
    want, _ = plain(ctx, cfg, trees, steps)
    n_sol = want[1]
    for cap in (1, 2, n_sol - 1, n_sol):
        info = {}
        r = forest_search(ctx, lb0, ub0, n_trees=trees, steps_per_launch=steps, capacity=64, collect_solutions=True, sink_capacity=cap, info=info,
                          **forest_kw(kind, brancher, val))
        in_forest = r["solutions"] - r["seeded_solutions"]
        print(name, kind, brancher, val, trees, steps, "capacity", cap, counts(r), "in the forest", in_forest, "drains", info.get("drains"), "launches", r["launches"])
        assert r["error"] == 0 and counts(r) == want
        check_set(ctx, cfg, r)
        if cap == 1:
            assert info["drains"] >= in_forest - 1
        if cap >= n_sol:
            assert info["drains"] == 0  # the new error is never raised
        if cap == n_sol - 1 and r["seeded_solutions"] == 0:
            assert info["drains"] == 1
    assert ctx_is_detached(ctx, kind)


def ctx_is_detached(ctx, kind):
    """After a collecting call the context has no sink: an entry that refuses one runs."""
    import pcp_amd.engine as E
    # (nothing is launched: a branch-and-bound entry looks at the sink first — PCP_ERR_UNSUPPORTED — and at its null buffers next — PCP_ERR_ARG)
    entry = ctx._L.pcp_dfs_forest_device_form_bnb if kind == "form" else ctx._L.pcp_dfs_forest_device_small_bnb
    st, obj = E.DfsState(), E.ForestObjective()
    return entry(ctx._h, C_.byref(st), 1, C_.byref(obj), 0, 0, None) == -1


def test_the_sink_is_detached_when_the_loop_raises(ctx):
    import pcp_amd.engine as E
    lb0, ub0 = push(ctx, "queens6")
    with pytest.raises(E.PcpError):  # capacity 1 < 2: refused by the entry, inside the loop, with the sink attached
        ctx.dfs_forest(lb0[None], ub0[None], capacity=1, small=True, collect_solutions=True)
    assert ctx_is_detached(ctx, "small")


# ------------------------------------------------------------------------------------------------ 3. the raw entry at a seam
class Raw:
    """T trees whose roots are given rows, the sink's buffers, and the C entries themselves."""

    def __init__(self, ctx, lbs, ubs, kind, brancher="split", val="middle", capacity=8, sink_rows=16):
        import torch
        import pcp_amd.engine as E
        self.E, self.ctx, self.torch, self.kind, self.enum = E, ctx, torch, kind, brancher == "enumerate"
        dev = torch.device("cuda", ctx.device)
        lbs, ubs = np.atleast_2d(lbs).astype(np.int32), np.atleast_2d(ubs).astype(np.int32)
        T, V = lbs.shape
        self.T, self.V, self.cap = T, V, capacity
        z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device=dev)
        self.lb, self.ub = z(T, capacity, V), z(T, capacity, V)
        self.lb[:, 0], self.ub[:, 0] = torch.from_numpy(lbs).to(dev), torch.from_numpy(ubs).to(dev)
        self.sp, self.stop = torch.ones(T, dtype=torch.int32, device=dev), z(T)
        self.status, self.counters = z(T, capacity, dt=torch.uint8), z(T, 5, dt=torch.int64)
        self.row_base, self.row_excl, self.path = z(T, capacity), z(T, capacity, 2), z(T, 4, 2)
        self.row_excl[:, :, 0] = -1
        self.val = E.VAL_MODES[val]
        self.s_lb, self.s_ub = torch.full((sink_rows, V), -77, dtype=torch.int32, device=dev), torch.full((sink_rows, V), -77, dtype=torch.int32, device=dev)
        self.s_tree, self.s_count = torch.full((sink_rows,), -77, dtype=torch.int32, device=dev), z(1)

    def sink(self, rows, **over):
        E = self.E
        s = E.PcpSolutionSink(self.s_lb.data_ptr(), self.s_ub.data_ptr(), self.s_tree.data_ptr(), self.s_count.data_ptr(), rows, 0)
        for k, v in over.items():
            setattr(s, k, v)
        return self.ctx._L.pcp_solution_sink_set(self.ctx._h, C_.byref(s))

    def detach(self):
        return self.ctx._L.pcp_solution_sink_set(self.ctx._h, None)

    def call(self, n_steps, stop_on_solution=0, node_limit=0):
        E, L, h = self.E, self.ctx._L, self.ctx._h
        st = E.DfsState(self.lb.data_ptr(), self.ub.data_ptr(), self.cap, self.sp.data_ptr(), self.stop.data_ptr(), self.status.data_ptr(), self.counters.data_ptr(),
                        None, None)
        if self.enum:
            x = E.ForestExcl(self.path.data_ptr(), self.row_base.data_ptr(), self.row_excl.data_ptr(), 4, self.val)
            rc = L.pcp_dfs_forest_device_small_enum(h, C_.byref(st), self.T, C_.byref(x), None, n_steps, stop_on_solution, node_limit, None)
        else:
            entry = L.pcp_dfs_forest_device_form if self.kind == "form" else L.pcp_dfs_forest_device_small
            rc = entry(h, C_.byref(st), self.T, n_steps, stop_on_solution, node_limit, None)
        self.torch.cuda.synchronize()
        return rc


@functools.lru_cache(maxsize=None)
def true_boxes(name):
    """The True nodes of the host BinarySplit search over the oracle stand-in: roots that are solutions at their first step."""
    k = K.KeepBoxes(K.stand_in(name))
    S.dfs(k, *K.root(name), all_solutions=True)
    return np.stack([b[0] for b in k.boxes]), np.stack([b[1] for b in k.boxes])


@pytest.mark.parametrize("cfg", [("sched3", "form", "split", "middle"), ("queens6", "small", "split", "middle"), ("queens6", "small", "enumerate", "middle"),
                                 ("golomb4", "small", "enumerate", "min")], ids=lambda c: "-".join(c))
def test_the_raw_entry_with_one_row_for_several_trees(ctx, cfg):
    name, kind, brancher, val = cfg
    push(ctx, name)
    lbs, ubs = true_boxes(name)
    lbs, ubs = lbs[-5:], ubs[-5:]  # (the schedule's last True nodes: one of them is a proper box)
    if name == "sched3":
        assert (lbs < ubs).any()
    T = len(lbs)
    raw = Raw(ctx, lbs, ubs, kind, brancher, val)
    enum = brancher == "enumerate"
    if enum:
        # every root arrives with an exclusion of its own that its bounds entail: popping it appends the entry to the path, and a row
        # handed back says so — it inherits one entry and appends none
        for t in range(T):
            raw.row_excl[t, 0, 0], raw.row_excl[t, 0, 1] = 0, int(ubs[t, 0]) + 1
    assert raw.sink(1) == 0
    try:
        assert raw.call(4) == 0
        cn = raw.counters.cpu().numpy()
        sp, stop = raw.sp.cpu().numpy(), raw.stop.cpu().numpy()
        assert int(raw.s_count[0]) == T  # every tree drew
        t0 = int(raw.s_tree[0])
        assert 0 <= t0 < T
        assert np.array_equal(raw.s_lb[0].cpu().numpy(), lbs[t0]) and np.array_equal(raw.s_ub[0].cpu().numpy(), ubs[t0])
        assert (raw.s_lb[1:] == -77).all() and (raw.s_ub[1:] == -77).all() and (raw.s_tree[1:] == -77).all()  # exactly one row was written
        assert cn[t0, :4].tolist() == [1, 1, 0, 0] and sp[t0] == 0 and stop[t0] == 0
        for t in range(T):
            if t == t0:
                continue
            assert cn[t, :4].tolist() == [0, 0, 0, 6] and stop[t] == 1 and sp[t] == 1, t
            assert np.array_equal(raw.lb[t, 0].cpu().numpy(), lbs[t]) and np.array_equal(raw.ub[t, 0].cpu().numpy(), ubs[t]), t
            if enum:
                assert int(raw.row_base[t, 0]) == 1 and raw.row_excl[t, 0].cpu().tolist() == [-1, 0], t
                assert raw.path[t, 0].cpu().tolist() == [0, int(ubs[t, 0]) + 1], t
        # the caller's part: the row is taken, the count zeroed, error and stop cleared — and a sink with room for all
        got_lb, got_ub = [raw.s_lb[0].cpu().numpy().copy()], [raw.s_ub[0].cpu().numpy().copy()]
        raw.s_count.zero_()
        raw.counters[:, 3] = 0
        raw.stop.zero_()
        assert raw.sink(T) == 0
        assert raw.call(4) == 0
        n = int(raw.s_count[0])
        assert n == T - 1
        got_lb += list(raw.s_lb[:n].cpu().numpy()); got_ub += list(raw.s_ub[:n].cpu().numpy())
        assert sorted(raw.s_tree[:n].cpu().tolist()) == [t for t in range(T) if t != t0]
        assert K.multiset(np.concatenate([np.array(got_lb), np.array(got_ub)], axis=1)) == K.multiset(np.concatenate([lbs, ubs], axis=1))
        cn = raw.counters.cpu().numpy()
        assert (cn[:, :4] == [1, 1, 0, 0]).all() and (raw.sp == 0).all()
    finally:
        assert raw.detach() == 0


# ------------------------------------------------------------------------------------------------ 4. the StopNode limit node
@pytest.mark.parametrize("cfg", LIGHT, ids=LIGHT_IDS)
def test_the_limit_node_is_counted_and_not_appended(ctx, cfg):
    name, kind, brancher, val = cfg
    lb0, ub0 = push(ctx, name)
    kw = forest_kw(kind, brancher, val)
    first = ctx.dfs_forest(lb0[None], ub0[None], stop_on_solution=True, steps_per_launch=256, capacity=64, **kw)
    k = first["nodes"]  # the first solution is node k
    assert first["solutions"] == 1 and k > 1
    r = ctx.dfs_forest(lb0[None], ub0[None], node_limit_per_tree=k, steps_per_launch=3, capacity=64, collect_solutions=True, sink_capacity=4, **kw)
    assert r["error"] == 0 and counts(r) == (k, 0, first["failed"]) and len(r["solutions_lb"]) == 0
    r = ctx.dfs_forest(lb0[None], ub0[None], node_limit_per_tree=k + 1, steps_per_launch=3, capacity=64, collect_solutions=True, sink_capacity=4, **kw)
    assert r["error"] == 0 and r["nodes"] == k + 1 and r["solutions"] == 1 and len(r["solutions_lb"]) == 1


# ------------------------------------------------------------------------------------------------ 5. stop_on_solution
@pytest.mark.parametrize("cfg", LIGHT, ids=LIGHT_IDS)
def test_stop_on_solution_appends_then_stops(ctx, cfg):
    from pcp_amd.search_forest import seed_roots_interval
    name, kind, brancher, val = cfg
    lb0, ub0 = push(ctx, name)
    kw = forest_kw(kind, brancher, val)
    seeded = seed_roots_interval(ctx, lb0, ub0, 4, **({} if brancher == "split" else dict(brancher=brancher, val=val)))
    rl, ru = seeded[0], seeded[1]
    if brancher == "enumerate":
        kw["root_excl"] = seeded[3]
    r = ctx.dfs_forest(rl, ru, stop_on_solution=True, want_solution=True, steps_per_launch=256, capacity=64, rebalance=False, collect_solutions=True, **kw)
    per = r["per_tree"]
    assert r["error"] == 0 and r["solutions"] >= 1 and (per[:, 1] <= 1).all()
    assert sorted(r["solution_tree"].tolist()) == [t for t in range(len(per)) if per[t, 1]]
    for row, t in zip(r["solutions_lb"], r["solution_tree"]):
        assert np.array_equal(row, r["first_solutions"][t])  # first_solution keeps the lower bounds of the same node
    sols = K.brute(name)
    assert all(p in sols for l, u in zip(r["solutions_lb"], r["solutions_ub"]) for p in K.points(l, u))


# ------------------------------------------------------------------------------------------------ 6. the refusals of the C ABI
def test_malformed_sinks_and_the_entries_that_refuse_one(ctx):
    import pcp_amd.engine as E
    lb0, ub0 = push(ctx, "golomb4")
    raw = Raw(ctx, lb0, ub0, "small")
    for over in (dict(lb=None), dict(ub=None), dict(count=None), dict(capacity=0), dict(reserved=1)):
        assert raw.sink(4, **over) == -1, over
    assert "pcp_solution_sink_set" in ctx._L.pcp_last_error(ctx._h).decode()
    assert ctx._L.pcp_solution_sink_set(None, None) == -1
    assert raw.sink(4, tree=None) == 0  # the tree column is optional
    # four rows fit, the fifth solution's ticket does not: *count exceeds the capacity by the one node handed back
    assert raw.call(256) == 0 and int(raw.s_count[0]) == 5 and (raw.s_tree == -77).all() and (raw.s_lb[4:] == -77).all()
    assert raw.counters[0, 1:4].cpu().tolist() == [4, raw.counters[0, 2].item(), 6] and int(raw.stop[0]) == 1
    assert raw.detach() == 0

    def refused(run):
        """-5 and a message that names the sink while one is attached; the same call runs once it is detached."""
        assert raw.sink(4) == 0
        try:
            with pytest.raises(E.PcpError) as e:
                run()
            assert e.value.code == -5 and "sink" in str(e.value)
        finally:
            assert raw.detach() == 0
        return run()

    var = K.GOLOMB_M - 1
    r = refused(lambda: ctx.dfs_forest_bnb(lb0[None], ub0[None], (var, "min"), steps_per_launch=64, capacity=64, small=True))
    assert r["best"] == 6
    r = refused(lambda: ctx.dfs_forest_bnb(lb0[None], ub0[None], (var, "min"), steps_per_launch=64, capacity=64, small=True, brancher="enumerate"))
    assert r["best"] == 6
    lb0, ub0 = push(ctx, "sched3")
    r = refused(lambda: ctx.dfs_forest_bnb(lb0[None], ub0[None], (0, "min"), steps_per_launch=64, capacity=64))
    assert r["best"] == 0
    lb0, ub0 = push(ctx, "queens6")
    r = refused(lambda: ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=64, capacity=64))  # the all-XNeqY forest
    assert counts(r) == K.SPLIT_TREE["queens6"][:3]
    props = M.lower_units([M.XNeqY(M.Identity(0), M.Identity(1)), M.XLessY(M.Identity(2), M.Identity(3))], 4)
    ctx.set_model(4, props, set_words=1)
    ctx.set_hull(0, 5)
    bits = M.interval_bits(np.zeros(4, np.int32), np.full(4, 5, np.int32), 1, 0)[None]
    plain_set = refused(lambda: ctx.dfs_forest_set(bits, steps_per_launch=64))
    enum_set = refused(lambda: ctx.dfs_forest_set(bits, steps_per_launch=64, brancher="enumerate"))
    assert plain_set["solutions"] == enum_set["solutions"] > 0 and plain_set["error"] == 0
    refused(lambda: ctx.dfs_forest_set_bnb(bits, (0, "min"), steps_per_launch=64))


# ------------------------------------------------------------------------------------------------ 7. expansion plus forest
@pytest.mark.parametrize("brancher,trees", [("split", 204), ("enumerate", 128)])
def test_forest_search_returns_the_expansions_solutions_too(ctx, brancher, trees):
    """N-queens 8 expanded to at least 128 open nodes: the expansion itself finds seven of the 92 solutions (computed on the oracle stand-in
    with the same DeviceSearch rounds) and leaves 204 roots under BinarySplit, 128 under Enumerate on MiddleVal."""
    from pcp_amd.search_forest import forest_search
    cfg = ("queens8", "small", brancher, "middle")
    lb0, ub0 = push(ctx, "queens8")
    info = {}
    r = forest_search(ctx, lb0, ub0, n_trees=128, steps_per_launch=64, capacity=64, collect_solutions=True, sink_capacity=16, info=info,
                      **forest_kw("small", brancher, "middle"))
    print("queens 8", brancher, counts(r), "trees", r["trees"], "seeded", r["seeded_solutions"], "drains", info.get("drains"))
    assert r["error"] == 0 and r["trees"] == trees and r["seeded_solutions"] == 7
    assert len(r["solutions_lb"]) == r["solutions"] == 92 and (r["solution_tree"] == -1).sum() == 7
    assert info["drains"] >= 1
    check_set(ctx, cfg, r)
