"""Enumerate in the small-store forest on the device (pcp_dfs_forest_device_small_enum; smalldfs_kernel<BNB, true>, pcp_smalldfs.hip): one
tree against the host specification's constants and, at every launch seam, against TreeSim's rows, row words and path; the stores of
small_forest_cases.py; expansion plus forest; workgroups with idle wavefronts; growth of stack and path, refill with the lists moving
along; error 5; malformed entries; branch and bound; N-queens-8; marks below zero under MinVal; the contract; BinarySplit untouched.
test_small_enum_forest_cpu.py pins the figures."""
import ctypes as C_

import numpy as np
import pytest

import small_enum_forest_cases as EC
import small_forest_cases as C
from pcp_amd import model as M
from pcp_amd import search as S
from test_small_enum_forest_cpu import ENUM_BNB, ENUM_TREE
from test_small_forest_cpu import GOLOMB_TREE

pytestmark = pytest.mark.gpu

NONE = -1  # row_excl[r].var == 0xFFFFFFFF as int32


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


def push(ctx, name):
    """Push the model; (lb0, ub0, objective variable)."""
    var = None
    if name.startswith("golomb") and "-" not in name:
        vs, cs, var = C.golomb(int(name[6:]))
    elif name == "golomb5-3":
        vs, cs = C.golomb_shifted(5, -3)
    elif name == "queens8":
        vs, cs = C.queens8()
    else:
        vs, cs = C.store(name)
    M.push_model(ctx, cs, len(vs))
    lb0, ub0 = vs.bounds()
    return np.ascontiguousarray(lb0, np.int32), np.ascontiguousarray(ub0, np.int32), var


def counts(r):
    return r["nodes"], r["solutions"], r["failed"]


class Raw:
    """The buffers of n trees and the C entry itself, one call per launch."""

    def __init__(self, ctx, lbs, ubs, capacity=64, path_capacity=128, val="middle", objective=None):
        import torch
        import pcp_amd.engine as E
        self.E, self.ctx, self.torch = E, ctx, torch
        dev = torch.device("cuda", ctx.device)
        lbs, ubs = np.atleast_2d(lbs).astype(np.int32), np.atleast_2d(ubs).astype(np.int32)
        T, V = lbs.shape
        self.T, self.V, self.cap = T, V, capacity
        z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device=dev)
        self.lb, self.ub = z(T, capacity, V), z(T, capacity, V)
        self.lb[:, 0], self.ub[:, 0] = torch.from_numpy(lbs).to(dev), torch.from_numpy(ubs).to(dev)
        self.sp, self.stop = torch.ones(T, dtype=torch.int32, device=dev), z(T)
        self.status, self.counters = z(T, capacity, dt=torch.uint8), z(T, 5, dt=torch.int64)
        self.row_base, self.row_excl = z(T, capacity), z(T, capacity, 2)
        self.row_excl[:, :, 0] = NONE
        self.val = E.VAL_MODES[val]
        self.set_path(path_capacity)
        self.obj = None
        if objective is not None:
            var, mode = objective
            self.best = torch.full((1,), E.no_incumbent(mode), dtype=torch.int32, device=dev)
            self.tree_best = torch.full((T,), E.no_incumbent(mode), dtype=torch.int32, device=dev)
            self.tree_row = z(T, V)
            self.obj = E.ForestObjective(var, E.OBJ_MODES[mode], self.best.data_ptr(), self.tree_best.data_ptr(), self.tree_row.data_ptr())

    def set_path(self, path_capacity):
        torch = self.torch
        old = getattr(self, "path", None)
        self.path = torch.zeros((self.T, max(path_capacity, 1), 2), dtype=torch.int32, device=self.lb.device)
        if old is not None:
            k = min(old.shape[1], self.path.shape[1])
            self.path[:, :k] = old[:, :k]
        self.path_capacity = path_capacity

    def call(self, n_steps, stop_on_solution=0, node_limit=0, ex=True, st_over=None, ex_over=None):
        E = self.E
        st = E.DfsState(self.lb.data_ptr(), self.ub.data_ptr(), self.cap, self.sp.data_ptr(), self.stop.data_ptr(), self.status.data_ptr(), self.counters.data_ptr(),
                        None, None)
        x = E.ForestExcl(self.path.data_ptr() if self.path_capacity else None, self.row_base.data_ptr(), self.row_excl.data_ptr(), self.path_capacity, self.val)
        for k, v in (ex_over or {}).items():
            setattr(x, k, v)
        for k, v in (st_over or {}).items():
            setattr(st, k, v)
        rc = self.ctx._L.pcp_dfs_forest_device_small_enum(self.ctx._h, C_.byref(st), self.T, C_.byref(x) if ex else None,
                                                          C_.byref(self.obj) if self.obj is not None else None, n_steps, stop_on_solution, node_limit, None)
        self.torch.cuda.synchronize()
        return rc

    def run(self, n_steps, max_launches=1 << 20):
        for _ in range(max_launches):
            assert self.call(n_steps) == 0
            if not ((self.sp > 0) & (self.stop == 0)).any():
                break
        return self.counters.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. one tree is the specification
@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("steps", [1, 5, 64])
def test_one_tree_is_the_specification_at_launch_seams(ctx, steps, val):
    lb0, ub0, _ = push(ctx, "golomb5")
    want = ENUM_TREE[("golomb5", val)]
    raw = Raw(ctx, lb0, ub0, val=val)
    if steps != 1:
        cn = raw.run(steps)
        print("golomb 5", val, steps, cn[0].tolist())
        assert tuple(cn[0, :3].tolist()) == want and cn[0, 3] == 0 and int(raw.sp[0]) == 0
        return
    sim = EC.TreeSim("golomb5", val)
    while sim.sp:
        assert raw.call(1) == 0
        sim.step()
        sp = int(raw.sp[0])
        assert sp == sim.sp and int(raw.counters[0, 0]) == sim.nodes, sim.nodes
        if sp:
            L, U, base, own, path = sim.top()
            assert np.array_equal(raw.lb[0, sp - 1].cpu().numpy(), L) and np.array_equal(raw.ub[0, sp - 1].cpu().numpy(), U), sim.nodes
            assert int(raw.row_base[0, sp - 1]) == base, sim.nodes
            got = raw.row_excl[0, sp - 1].cpu().numpy()
            assert (int(got[0]) & 0xFFFFFFFF, int(got[1]) if got[0] != NONE else 0) == own, sim.nodes
            assert [tuple(p) for p in raw.path[0, :base].cpu().numpy().tolist()] == path, sim.nodes
    assert plan_is_small(ctx, 1)
    cn = raw.counters.cpu().numpy()
    assert tuple(cn[0, :3].tolist()) == want == (sim.nodes, sim.solutions, sim.failed) and cn[0, 3] == 0


def plan_is_small(ctx, grid):
    p = ctx.last_plan()
    return p["path"] == 4 and p["grid"] == grid and p["block"] == 256


@pytest.mark.parametrize("val", ["middle", "min"])
def test_golomb6_one_tree(ctx, val):
    lb0, ub0, _ = push(ctx, "golomb6")
    r = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=64, capacity=64, small=True, brancher="enumerate", val=val)
    print("golomb 6", val, counts(r))
    assert r["error"] == 0 and r["open"] == 0 and counts(r) == ENUM_TREE[("golomb6", val)]


# ------------------------------------------------------------------------------------------------ 2. stores
@pytest.mark.parametrize("name", sorted(C.STORES))
def test_stores_against_the_host_specification(ctx, name):
    lb0, ub0, _ = push(ctx, name)
    want = S.dfs_enumerate(ctx, lb0, ub0, all_solutions=True, batch=1, node_limit=C.NODE_LIMIT, val="middle")
    r = ctx.dfs_forest(lb0[None], ub0[None], node_limit_per_tree=C.NODE_LIMIT, steps_per_launch=256, capacity=512, small=True, brancher="enumerate")
    print("store", name, counts(r), EC.counts(want))
    assert ctx.last_plan()["path"] == 4
    assert r["error"] == 0 and counts(r) == EC.counts(want)


# ------------------------------------------------------------------------------------------------ 3. expansion plus forest
@pytest.mark.parametrize("trees", [3, 5, 64])
def test_expansion_plus_forest_is_the_complete_tree(ctx, trees):
    from pcp_amd.search_forest import forest_search, seed_roots_interval
    lb0, ub0, _ = push(ctx, "golomb6")
    rl, ru, st, lists = seed_roots_interval(ctx, lb0, ub0, trees, brancher="enumerate", val="middle")
    assert len(lists) == rl.shape[0] >= trees and any(len(e) for e in lists)
    info = {}
    r = forest_search(ctx, lb0, ub0, n_trees=trees, steps_per_launch=64, capacity=64, small=True, brancher="enumerate", val="middle", info=info)
    plan = ctx.last_plan()
    print("golomb 6 enumerate forest", trees, counts(r), "trees", r["trees"], "steals", info.get("steals"))
    assert r["error"] == 0 and counts(r) == ENUM_TREE[("golomb6", "middle")] and r["trees"] == rl.shape[0]
    assert plan["path"] == 4 and plan["block"] == 256 and plan["grid"] == -(-r["trees"] // 4)
    one = ctx.dfs_forest(rl, ru, steps_per_launch=256, capacity=64, small=True, brancher="enumerate", root_excl=lists, want_solution=True)
    for t in range(rl.shape[0]):
        if one["per_tree"][t, 1]:
            assert C.is_ruler(one["first_solutions"][t], 6), t


def test_a_workgroup_with_three_trees_and_one_with_a_finished_tree(ctx):
    """Three roots: the fourth wavefront has no tree.  Then four trees of which one starts with an empty stack.  Nobody waits."""
    from pcp_amd.search_forest import seed_roots_interval
    import torch
    lb0, ub0, _ = push(ctx, "golomb5")
    rl, ru, st, lists = seed_roots_interval(ctx, lb0, ub0, 3, brancher="enumerate", val="middle")
    rl, ru, lists = rl[:3], ru[:3], lists[:3]
    r = ctx.dfs_forest(rl, ru, steps_per_launch=4096, capacity=64, rebalance=False, small=True, brancher="enumerate", root_excl=lists)
    assert plan_is_small(ctx, 1) and r["error"] == 0 and r["open"] == 0
    for t in range(3):  # each tree alone gives the same
        alone = ctx.dfs_forest(rl[t:t + 1], ru[t:t + 1], steps_per_launch=4096, capacity=64, small=True, brancher="enumerate", root_excl=lists[t:t + 1])
        assert counts(alone) == tuple(r["per_tree"][t, :3].tolist()), t
    rl4, ru4 = torch.cat([rl[:1], rl[:1], rl[1:]]), torch.cat([ru[:1], ru[:1], ru[1:]])
    e = ctx.dfs_forest(rl4, ru4, steps_per_launch=4096, capacity=64, sp0=[1, 0, 1, 1], rebalance=False, small=True, brancher="enumerate",
                       root_excl=[lists[0], lists[0], lists[1], lists[2]])
    assert plan_is_small(ctx, 1) and e["error"] == 0 and e["open"] == 0 and e["per_tree"][1, 0] == 0
    assert np.array_equal(e["per_tree"][[0, 2, 3], :3], r["per_tree"][:, :3])


# ------------------------------------------------------------------------------------------------ 4. growth and refill
def test_growth_and_refill(ctx):
    """Two-row stacks and a one-entry path, eight nodes per launch, every open node of the expansion a tree: the stacks and the paths grow,
    finished trees steal, and expansion plus forest is still the complete tree.  The first steal is looked at: the receiver's row 0 under
    its path is the donor's former bottom node."""
    from pcp_amd.search_forest import seed_roots_interval
    lb0, ub0, _ = push(ctx, "golomb6")
    rl, ru, st, lists = seed_roots_interval(ctx, lb0, ub0, 5, brancher="enumerate", val="middle")
    assert rl.shape[0] >= 5
    info = {}
    r = ctx.dfs_forest(rl, ru, steps_per_launch=8, capacity=2, max_capacity=256, path_capacity=1, small=True, brancher="enumerate", root_excl=lists, info=info)
    got = (r["nodes"] + st.num_nodes, r["solutions"] + st.num_solution, r["failed"] + st.num_failed_node)
    print("growth and refill", got, {k: info[k] for k in ("grown", "path_grown", "steals", "capacity", "path_capacity", "launches")})
    assert r["error"] == 0 and r["open"] == 0 and got == ENUM_TREE[("golomb6", "middle")]
    assert info["grown"] > 0 and info["path_grown"] > 0 and info["steals"] > 0
    fs = info["first_steal"]
    (bl, bu, be), (al, au, ae) = fs["before"], fs["after"]
    assert fs["donor"] != fs["receiver"] and np.array_equal(bl, al) and np.array_equal(bu, au)
    assert {tuple(p) for p in be.tolist()} == {tuple(p) for p in ae.tolist()}


# ------------------------------------------------------------------------------------------------ 5. error 5
def test_error_5_leaves_the_row_alone(ctx):
    """Under MinVal, where the path never grows beyond what the root brings: one entry."""
    lb0, ub0, _ = push(ctx, "golomb5")
    # a root with an interior exclusion of its own: the first mark above zero cannot be 5
    x, v = 1, 5
    assert lb0[x] < v < ub0[x]
    raw = Raw(ctx, lb0, ub0, path_capacity=0, val="min")
    raw.row_excl[0, 0, 0], raw.row_excl[0, 0, 1] = x, v
    assert raw.call(64) == 0  # an ordinary status return
    cn = raw.counters.cpu().numpy()[0]
    assert int(raw.sp[0]) == 1 and int(raw.stop[0]) == 1 and cn[:4].tolist() == [0, 0, 0, 5]
    assert np.array_equal(raw.lb[0, 0].cpu().numpy(), lb0) and np.array_equal(raw.ub[0, 0].cpu().numpy(), ub0)
    assert raw.row_excl[0, 0].cpu().tolist() == [x, v] and int(raw.row_base[0, 0]) == 0
    # resumed with a longer path: the one-tree result of that root
    raw.set_path(4)
    raw.counters[0, 3] = 0
    raw.stop[0] = 0
    cn = raw.run(64)[0]
    one = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=64, capacity=64, small=True, brancher="enumerate", val="min", root_excl=[np.array([[x, v]], np.int32)])
    sim = EC.TreeSim("golomb5", "min", root_excl=[(x, v)])
    print("error 5 resumed", cn.tolist(), counts(one))
    assert cn[3] == 0 and int(raw.sp[0]) == 0 and tuple(cn[:3].tolist()) == counts(one) == sim.run()
    # the loop does the same by itself: path_capacity = 0 grows
    info = {}
    raw2 = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=64, capacity=64, small=True, brancher="enumerate", path_capacity=0, info=info)
    assert raw2["error"] == 0 and counts(raw2) == ENUM_TREE[("golomb5", "middle")] and info["path_grown"] > 0
    low = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=64, capacity=64, small=True, brancher="enumerate", path_capacity=0, max_path=0)
    assert low["error"] == 5 and low["open"] > 0


# ------------------------------------------------------------------------------------------------ 6. malformed entries
def test_a_malformed_entry_stops_its_tree_alone(ctx):
    import pcp_amd.engine as E
    lb0, ub0, _ = push(ctx, "golomb5")
    V = len(lb0)
    want = ENUM_TREE[("golomb5", "middle")]
    ctx.stats_read()
    for where in ("path", "row"):
        raw = Raw(ctx, np.stack([lb0, lb0]), np.stack([ub0, ub0]))
        if where == "path":
            raw.path[0, 0, 0], raw.path[0, 0, 1] = V, 3
            raw.row_base[0, 0] = 1
        else:
            raw.row_excl[0, 0, 0], raw.row_excl[0, 0, 1] = V, 3
        cn = raw.run(4096)
        print("malformed", where, cn.tolist())
        assert cn[0, :4].tolist() == [1, 0, 0, 2] and int(raw.stop[0]) == 1 and int(raw.sp[0]) == 0
        assert tuple(cn[1, :3].tolist()) == want and cn[1, 3] == 0
        with pytest.raises(E.PcpError) as e:  # the sticky violation word; reading it reports and clears it
            ctx.stats_read()
        assert e.value.code == -2
        ctx.stats_read()


# ------------------------------------------------------------------------------------------------ 7. branch and bound
@pytest.mark.parametrize("name,val,mode", sorted(ENUM_BNB))
def test_one_tree_of_branch_and_bound_is_the_host_specification(ctx, name, val, mode):
    lb0, ub0, var = push(ctx, name)
    best, want = ENUM_BNB[(name, val, mode)]
    r = ctx.dfs_forest_bnb(lb0[None], ub0[None], (var, mode), steps_per_launch=64, capacity=64, small=True, brancher="enumerate", val=val)
    print(name, val, mode, counts(r), r["best"])
    assert ctx.last_plan()["path"] == 4
    assert r["error"] == 0 and r["open"] == 0 and counts(r) == want and r["best"] == best
    assert int(r["best_solution"][var]) == best and C.is_ruler(r["best_solution"], int(name[6]))
    if name == "golomb5":  # ... and the specification run on this context
        host = S.dfs_enumerate(ctx, lb0, ub0, batch=1, val=val, objective=(var, mode))
        assert (host.best, EC.counts(host)) == (best, want)


@pytest.mark.parametrize("trees", [3, 64])
def test_a_forest_of_branch_and_bound_finds_the_optimum(ctx, trees):
    from pcp_amd.search_forest import forest_bnb
    for m in (5, 6):
        lb0, ub0, var = push(ctx, f"golomb{m}")
        for val in ("middle", "min"):
            r = forest_bnb(ctx, lb0, ub0, (var, "min"), n_trees=trees, steps_per_launch=32, capacity=64, small=True, brancher="enumerate", val=val)
            print("golomb", m, trees, val, counts(r), r["best"])
            assert r["error"] == 0 and r["open"] == 0 and r["best"] == C.OPTIMUM[m] and r["nodes"] > 0
            row = np.asarray(r["best_solution"], np.int32)
            assert int(row[var]) == C.OPTIMUM[m] and C.is_ruler(row, m)


# ------------------------------------------------------------------------------------------------ 8. N-queens-8, marks below zero
@pytest.mark.parametrize("val", ["middle", "min"])
def test_queens8(ctx, val):
    lb0, ub0, _ = push(ctx, "queens8")
    r = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=256, capacity=64, small=True, brancher="enumerate", val=val)
    assert ctx.last_plan()["path"] == 4
    assert r["error"] == 0 and counts(r) == ENUM_TREE[("queens8", val)] and r["solutions"] == 92


def test_marks_below_zero_under_minval(ctx):
    """MinVal's value is a bound: none of MiddleVal's truncation toward zero, the tree ends."""
    lb0, ub0, _ = push(ctx, "golomb5-3")
    r = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=64, capacity=64, small=True, brancher="enumerate", val="min")
    print("golomb 5 from -3, MinVal", counts(r))
    assert r["error"] == 0 and r["open"] == 0 and counts(r) == ENUM_TREE[("golomb5-3", "min")]


# ------------------------------------------------------------------------------------------------ 9. contract
def test_contract(ctx):
    import pcp_amd.engine as E
    import form_forest_cases as FC
    lb0, ub0, var = push(ctx, "golomb5")
    raw = Raw(ctx, lb0, ub0, capacity=16, objective=(var, "min"))
    assert raw.call(0) == 0 and int(raw.counters[0, 0]) == 0 and int(raw.sp[0]) == 1  # n_steps = 0: PCP_OK, nothing is launched
    assert raw.call(0, ex=False) == -1
    assert raw.call(0, ex_over={"val": 2}) == -1
    assert raw.call(0, ex_over={"row_base": None}) == -1 and raw.call(0, ex_over={"row_excl": None}) == -1
    assert raw.call(0, ex_over={"path": None}) == -1                       # path_capacity > 0 and no path
    assert raw.call(0, ex_over={"path": None, "path_capacity": 0}) == 0
    assert raw.call(0, st_over={"capacity": 1}) == -1 and raw.call(0, st_over={"lb": None}) == -1 and raw.call(0, st_over={"counters": None}) == -1
    raw.T = 0
    assert raw.call(0) == -1
    raw.T = 1
    for bad in (E.ForestObjective(len(lb0), 0, raw.best.data_ptr(), raw.tree_best.data_ptr(), None), E.ForestObjective(var, 2, raw.best.data_ptr(), raw.tree_best.data_ptr(), None),
                E.ForestObjective(var, 0, None, raw.tree_best.data_ptr(), None), E.ForestObjective(var, 0, raw.best.data_ptr(), None, None)):
        raw.obj = bad
        assert raw.call(0) == -1
    raw.obj = None
    assert raw.call(0) == 0
    # stop_on_solution without an objective stops at the first solution; with one it is ignored
    one = ctx.dfs_forest(lb0[None], ub0[None], stop_on_solution=True, want_solution=True, steps_per_launch=64, capacity=64, small=True, brancher="enumerate")
    assert one["solutions"] == 1 and C.is_ruler(one["first_solutions"][0], 5)
    rb = Raw(ctx, lb0, ub0, objective=(var, "min"))
    for _ in range(1 << 16):
        assert rb.call(64, stop_on_solution=1) == 0
        if not ((rb.sp > 0) & (rb.stop == 0)).any():
            break
    assert tuple(rb.counters[0, :3].cpu().tolist()) == ENUM_BNB[("golomb5", "middle", "min")][1] and int(rb.best[0]) == C.OPTIMUM[5]
    # the stores one step beyond the limits, a store with formula units, a set-mode model
    for f in (C.slots129, C.recs2049):
        vs, cs = f()
        M.push_model(ctx, cs, len(vs))
        l0, u0 = vs.bounds()
        with pytest.raises(E.PcpError) as e:
            ctx.dfs_forest(l0[None], u0[None], capacity=16, small=True, brancher="enumerate")
        assert e.value.code == -5 and "pcp_dfs_forest_device_small_enum" in str(e.value)
    vs, cs, _ = FC.schedule("A4")
    M.push_model(ctx, cs, len(vs))
    l0, u0 = vs.bounds()
    with pytest.raises(E.PcpError) as e:
        ctx.dfs_forest(l0[None], u0[None], capacity=16, small=True, brancher="enumerate")
    assert e.value.code == -5
    props = M.lower_units([M.XNeqY(M.Identity(0), M.Identity(1)), M.XLessY(M.Identity(2), M.Identity(3))], 4)
    ctx.set_model(4, props, set_words=1)
    ctx.set_hull(0, 5)
    with pytest.raises(E.PcpError) as e:
        ctx.dfs_forest(np.zeros((2, 4), np.int32), np.full((2, 4), 5, np.int32), capacity=16, small=True, brancher="enumerate")
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------ 10. BinarySplit untouched
def test_binary_split_is_untouched(ctx):
    lb0, ub0, _ = push(ctx, "golomb5")
    r = ctx.dfs_forest(lb0[None], ub0[None], steps_per_launch=64, capacity=64, small=True)
    assert r["error"] == 0 and counts(r) == GOLOMB_TREE[5]
