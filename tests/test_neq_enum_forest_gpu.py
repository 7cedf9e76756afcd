"""Enumerate in the all-XNeqY forest on the device (pcp_dfs_forest_device_neq_enum; neqfix_kernel<.., DFS, .., EXCL>, pcp_neq.hip): one tree
against search.dfs_enumerate on the same context and against the figures test_neq_enum_forest_cpu.py pins; at every launch seam against
TreeSim's rows, row words and path; growth of stack and path, errors 1 and 5; several trees with steals; stores beyond the small-store
limits and wider than the workgroup; both instantiations; StopNode and the first solution; malformed input; the refusals of the C entry.

The launcher picks between two instantiations by the STORE, not by an option: cells are int2 always (as in pcp_dfs_forest_device), and the
payload format is 4 bytes per adjacency entry unless the store holds an offset beyond +-32767 — then 8 bytes.  N-queens runs the first, the
store of `wide_offset` the second."""
import ctypes as C_

import numpy as np
import pytest

import neq_enum_forest_cases as NC
from pcp_amd import model as M
from pcp_amd import search as S
from test_neq_enum_forest_cpu import ENUM_TREE

pytestmark = pytest.mark.gpu

NONE = -1  # row_excl[r].var == 0xFFFFFFFF as int32
QUEENS8_SPLIT = (779, 92, 298)  # BinarySplit's tree of N-queens-8 (test_small_forest_cpu.QUEENS8)


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


def counts(r):
    return r["nodes"], r["solutions"], r["failed"]


def host(ctx, lb0, ub0, val, **kw):
    st = S.dfs_enumerate(ctx, lb0, ub0, all_solutions=kw.pop("all_solutions", True), batch=1, val=val, **kw)
    return (st.num_nodes, st.num_solution, st.num_failed_node), st


def plan_is_neq(ctx, grid):
    p = ctx.last_plan()
    return p["path"] == 1 and p["grid"] == grid and p["nodes_per_block"] == 1 and p["packed"] == 0


class Raw:
    """The buffers of n trees — `dirty` rows included — and the C entry itself, one call per launch."""

    def __init__(self, ctx, lbs, ubs, capacity=64, path_capacity=128, val="middle"):
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
        self.row_base, self.row_excl = z(T, capacity), z(T, capacity, 2)
        self.row_excl[:, :, 0] = NONE
        self.val = E.VAL_MODES[val]
        self.path = None
        self.set_path(path_capacity)
        self.obj = None

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
        """More stack rows per tree; the rows, their status, hint and two words stay where they are."""
        def wider(t, fill=0):
            n = self.torch.full((t.shape[0], capacity) + tuple(t.shape[2:]), fill, dtype=t.dtype, device=self.dev)
            n[:, :self.cap] = t
            return n
        self.lb, self.ub, self.status, self.row_base = wider(self.lb), wider(self.ub), wider(self.status), wider(self.row_base)
        self.dirty, self.row_excl = wider(self.dirty, -1), wider(self.row_excl, -1)
        self.cap = capacity

    def call(self, n_steps, stop_on_solution=0, node_limit=0, ex=True, st=True, st_over=None, ex_over=None):
        E = self.E
        s = E.DfsState(self.lb.data_ptr(), self.ub.data_ptr(), self.cap, self.sp.data_ptr(), self.stop.data_ptr(), self.status.data_ptr(), self.counters.data_ptr(),
                       None, self.dirty.data_ptr())
        x = E.ForestExcl(self.path.data_ptr() if self.path_capacity else None, self.row_base.data_ptr(), self.row_excl.data_ptr(), self.path_capacity, self.val)
        for k, v in (ex_over or {}).items():
            setattr(x, k, v)
        for k, v in (st_over or {}).items():
            setattr(s, k, v)
        rc = self.ctx._L.pcp_dfs_forest_device_neq_enum(self.ctx._h, C_.byref(s) if st else None, self.T, C_.byref(x) if ex else None,
                                                        C_.byref(self.obj) if self.obj is not None else None, n_steps, stop_on_solution, node_limit, None)
        self.torch.cuda.synchronize()
        return rc

    def run(self, n_steps, max_launches=1 << 16):
        for _ in range(max_launches):
            assert self.call(n_steps) == 0
            if not ((self.sp > 0) & (self.stop == 0)).any():
                break
        return self.counters.cpu().numpy()

    def resume(self, t=0):
        self.counters[t, 3] = 0
        self.stop[t] = 0

    def same_as(self, sim, t=0):
        """sp, every open row, its two words and the top row's path prefix are TreeSim's."""
        sp = int(self.sp[t])
        assert sp == sim.sp and int(self.counters[t, 0]) == sim.nodes, (sp, sim.sp, sim.nodes)
        if not sp:
            return
        lb, ub = self.lb[t, :sp].cpu().numpy(), self.ub[t, :sp].cpu().numpy()
        base, own = self.row_base[t, :sp].cpu().numpy(), self.row_excl[t, :sp].cpu().numpy()
        for r in range(sp):
            assert np.array_equal(lb[r], sim.rows[r][0]) and np.array_equal(ub[r], sim.rows[r][1]), (sim.nodes, r)
            assert int(base[r]) == sim.row_base[r], (sim.nodes, r)
            e = sim.row_excl[r]
            assert (int(own[r, 0]), int(own[r, 1]) if own[r, 0] != NONE else 0) == (e if e is not None else (NONE, 0)), (sim.nodes, r)
        top = sim.row_base[sp - 1]
        assert [tuple(p) for p in self.path[t, :top].cpu().numpy().tolist()] == sim.path[:top], sim.nodes


# ------------------------------------------------------------------------------------------------ 4. one tree
@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("n", NC.SIZES)
def test_one_tree_is_dfs_enumerate_at_batch_one(ctx, n, val):
    lb0, ub0 = NC.push(ctx, n)
    want, _ = host(ctx, lb0, ub0, val)
    r = ctx.dfs_forest_enum(lb0[None], ub0[None], val=val, steps_per_launch=64, capacity=64, forest="neq")
    assert plan_is_neq(ctx, 1)
    plain = ctx.dfs_forest_enum(lb0[None], ub0[None], val=val, steps_per_launch=64, capacity=64, forest="neq", hints=False)
    print("queens", n, val, counts(r), want, counts(plain))
    assert r["error"] == 0 and r["open"] == 0 and counts(r) == want == ENUM_TREE[(n, val)] and r["solutions"] == NC.SOLUTIONS[n]
    assert plain["error"] == 0 and counts(plain) == counts(r)


# ------------------------------------------------------------------------------------------------ 5. seams
@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("steps", [1, 2, 3, 7])
def test_every_launch_seam_is_the_simulators_state(ctx, steps, val):
    lb0, ub0 = NC.push(ctx, 6)
    raw = Raw(ctx, lb0, ub0, val=val)
    sim = NC.TreeSim(6, val)
    while sim.sp:
        assert raw.call(steps) == 0
        for _ in range(steps):
            if sim.sp:
                sim.step()
        raw.same_as(sim)
    cn = raw.counters.cpu().numpy()[0]
    whole = Raw(ctx, lb0, ub0, val=val).run(512)[0]
    print("seams", steps, val, cn.tolist(), whole.tolist())
    assert tuple(cn[:3].tolist()) == tuple(whole[:3].tolist()) == ENUM_TREE[(6, val)] == (sim.nodes, sim.solutions, sim.failed) and cn[3] == whole[3] == 0
    # ... and through the driver: the open rows `info` names after k launches are the simulator's after k * steps nodes
    for k in (1, 4, 9):
        info = {}
        r = ctx.dfs_forest_enum(lb0[None], ub0[None], val=val, steps_per_launch=steps, capacity=64, forest="neq", max_launches=k, info=info)
        sim = NC.TreeSim(6, val)
        for _ in range(k * steps):
            if sim.sp:
                sim.step()
        assert r["nodes"] == sim.nodes and r["open"] == sim.sp and len(info["rows"][0][0]) == sim.sp
        for row in range(sim.sp):
            assert np.array_equal(info["rows"][0][0][row], sim.rows[row][0]) and np.array_equal(info["rows"][0][1][row], sim.rows[row][1]), (k, row)


# ------------------------------------------------------------------------------------------------ 6. growth, errors 5 and 1
@pytest.mark.parametrize("path_capacity", [0, 1])
def test_stack_and_path_grow_in_the_driver(ctx, path_capacity):
    lb0, ub0 = NC.push(ctx, 8)
    info = {}
    r = ctx.dfs_forest_enum(lb0[None], ub0[None], steps_per_launch=16, capacity=2, max_capacity=256, path_capacity=path_capacity, forest="neq", info=info)
    print("growth", path_capacity, counts(r), {k: info[k] for k in ("grown", "path_grown", "capacity", "path_capacity", "launches")})
    assert r["error"] == 0 and r["open"] == 0 and counts(r) == ENUM_TREE[(8, "middle")]
    assert info["path_grown"] > 0 and info["grown"] > 0


def test_errors_5_and_1_leave_the_row_on_the_stack_uncounted(ctx):
    lb0, ub0 = NC.push(ctx, 6)
    want = ENUM_TREE[(6, "middle")]
    # error 5: no path at all — the first row popped with an entry of its own stays, and nothing of the state has moved
    raw = Raw(ctx, lb0, ub0, path_capacity=0)
    assert raw.call(512) == 0
    cn = raw.counters.cpu().numpy()[0]
    assert cn[3] == 5 and int(raw.stop[0]) == 1 and 0 < cn[0] < want[0]
    sim = NC.TreeSim(6)
    for _ in range(int(cn[0])):
        sim.step()
    raw.same_as(sim)
    assert sim.row_excl[-1] is not None and sim.row_base[-1] == 0  # the row it stopped at has an entry, and the path no room
    assert raw.call(512) == 0 and raw.counters.cpu().numpy()[0].tolist() == cn.tolist()  # stopped: another call changes nothing
    raw.set_path(16)
    raw.resume()
    cn = raw.run(512)[0]
    assert tuple(cn[:3].tolist()) == want and cn[3] == 0 and int(raw.sp[0]) == 0
    # error 1: two rows — the node that cannot push its children stays on top, propagated and uncounted, its list in the path
    raw = Raw(ctx, lb0, ub0, capacity=2)
    assert raw.call(512) == 0
    cn = raw.counters.cpu().numpy()[0]
    sp = int(raw.sp[0])
    assert cn[3] == 1 and int(raw.stop[0]) == 1 and sp == 2 and 0 < cn[0] < want[0]
    sim = NC.TreeSim(6)
    for _ in range(int(cn[0])):
        sim.step()
    assert sim.sp == sp  # the node on top is the simulator's next one: not yet counted
    L, U, base, own, _ = sim.top()
    assert int(raw.row_base[0, sp - 1]) == base + (own[0] != NC.NONE) and int(raw.row_excl[0, sp - 1, 0]) == NONE
    top_l, top_u = raw.lb[0, sp - 1].cpu().numpy(), raw.ub[0, sp - 1].cpu().numpy()
    assert (top_l >= L).all() and (top_u <= U).all()  # (propagated: inside the simulator's unpropagated row)
    raw.set_capacity(64)
    raw.resume()
    cn = raw.run(512)[0]
    print("errors 5 and 1 resumed", cn.tolist())
    assert tuple(cn[:3].tolist()) == want and cn[3] == 0 and int(raw.sp[0]) == 0


# ------------------------------------------------------------------------------------------------ 7. several trees
@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("trees", [5, 64])
def test_expansion_plus_forest_is_the_complete_tree(ctx, trees, val):
    from pcp_amd.search_forest import forest_enumerate
    lb0, ub0 = NC.push(ctx, 8)
    info = {}
    r = forest_enumerate(ctx, lb0, ub0, val=val, n_trees=trees, steps_per_launch=8, forest="neq", capacity=4, path_capacity=1, info=info)
    print("queens 8 forest", trees, val, counts(r), "trees", r["trees"], "steals", info.get("steals"), "grown", info.get("grown"), info.get("path_grown"))
    assert r["error"] == 0 and counts(r) == ENUM_TREE[(8, val)] and r["trees"] >= trees
    assert plan_is_neq(ctx, r["trees"])
    assert info["steals"] > 0


# ------------------------------------------------------------------------------------------------ 8. beyond the small limits
def test_a_store_beyond_the_small_limits_goes_to_the_all_xneqy_kernel_by_itself(ctx):
    import pcp_amd.engine as E
    n = 40
    ctx.set_model(n, M.nqueens_props(n))
    assert ctx.n_props == 2340 and ctx.all_neq and ctx.beyond_small_limits
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    for val in ("middle", "min"):
        want, _ = host(ctx, lb0, ub0, val, node_limit=400)
        r = ctx.dfs_forest_enum(lb0[None], ub0[None], val=val, node_limit_per_tree=400, steps_per_launch=128, capacity=512)
        print("queens 40", val, counts(r), want)
        assert plan_is_neq(ctx, 1) and ctx.last_plan()["block"] == 512
        assert r["error"] == 0 and counts(r) == want and r["nodes"] == 400
    with pytest.raises(E.PcpError) as e:  # the small-store entry, forced, still refuses it
        ctx.dfs_forest_enum(lb0[None], ub0[None], node_limit_per_tree=4, capacity=16, forest="small")
    assert e.value.code == -5
    lb8, ub8 = NC.push(ctx, 8)  # ... and a small store keeps the small-store forest
    assert not ctx.beyond_small_limits
    r = ctx.dfs_forest_enum(lb8[None], ub8[None], steps_per_launch=256, capacity=64)
    assert ctx.last_plan()["path"] == 4 and counts(r) == ENUM_TREE[(8, "middle")]


@pytest.mark.parametrize("val", ["middle", "min"])
def test_more_variables_than_the_workgroup_has_threads(ctx, val):
    n = 600
    ctx.set_model(n, M.nqueens_props(n))
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    want, _ = host(ctx, lb0, ub0, val, node_limit=64)
    r = ctx.dfs_forest_enum(lb0[None], ub0[None], val=val, node_limit_per_tree=64, steps_per_launch=16, capacity=128)
    print("queens 600", val, counts(r), want)
    assert plan_is_neq(ctx, 1) and ctx.last_plan()["block"] == 512 < n
    assert r["error"] == 0 and counts(r) == want and r["nodes"] == 64


def wide_offset(n):
    """N-queens-n plus one record whose offset does not fit 16 bits — it can never act, the tree is N-queens-n's, but the store's adjacency
    payloads are the 8-byte ones."""
    vs, cs = M.nqueens(n)
    cs.alloc(M.XNeqY(M.Identity(0), M.Addition(M.Identity(1), 40000)))
    return vs, cs


@pytest.mark.parametrize("val", ["middle", "min"])
def test_the_eight_byte_payload_instantiation(ctx, val):
    vs, cs = wide_offset(6)
    M.push_model(ctx, cs, len(vs))
    assert ctx.all_neq
    lb0, ub0 = (np.ascontiguousarray(a, np.int32) for a in vs.bounds())
    want, _ = host(ctx, lb0, ub0, val)
    r = ctx.dfs_forest_enum(lb0[None], ub0[None], val=val, steps_per_launch=7, capacity=64, forest="neq")
    assert plan_is_neq(ctx, 1)
    assert r["error"] == 0 and counts(r) == want == ENUM_TREE[(6, val)]


# ------------------------------------------------------------------------------------------------ 9. StopNode, the first solution
@pytest.mark.parametrize("val", ["middle", "min"])
def test_the_limit_node_is_neither_a_solution_nor_a_failure(ctx, val):
    lb0, ub0 = NC.push(ctx, 6)
    sim, cum = NC.TreeSim(6, val), [(0, 0, 0)]
    kinds = {}
    while sim.sp:
        sim.step()
        cum.append((sim.nodes, sim.solutions, sim.failed))
        kinds.setdefault(sim.last[3], sim.nodes)  # the first node of each status (0 failed, 1 solution, 2 unknown)
    assert set(kinds) == {0, 1, 2}
    for status, limit in sorted(kinds.items()):
        r = ctx.dfs_forest_enum(lb0[None], ub0[None], val=val, node_limit_per_tree=limit, steps_per_launch=5, capacity=64, forest="neq")
        want, _ = host(ctx, lb0, ub0, val, node_limit=limit)
        print("limit", val, status, limit, counts(r), want)
        assert counts(r) == want == (limit,) + cum[limit - 1][1:] and r["error"] == 0


@pytest.mark.parametrize("val", ["middle", "min"])
def test_the_first_solution_is_dfs_enumerates(ctx, val):
    lb0, ub0 = NC.push(ctx, 8)
    want, st = host(ctx, lb0, ub0, val, all_solutions=False)
    r = ctx.dfs_forest_enum(lb0[None], ub0[None], val=val, stop_on_solution=True, want_solution=True, steps_per_launch=16, capacity=64, forest="neq")
    assert r["solutions"] == 1 == want[1] and counts(r) == want
    assert np.array_equal(r["first_solutions"][0], st.solutions[0]) and NC.is_queens(r["first_solutions"][0], 8)


# ------------------------------------------------------------------------------------------------ 10. malformed input
@pytest.mark.parametrize("where", ["path", "row", "base"])
def test_malformed_input_stops_its_tree_alone(ctx, where):
    import pcp_amd.engine as E
    lb0, ub0 = NC.push(ctx, 6)
    V = len(lb0)
    ctx.stats_read()
    raw = Raw(ctx, np.stack([lb0, lb0]), np.stack([ub0, ub0]), path_capacity=16)
    if where == "path":    # a root list with var = n_vars
        raw.path[0, 0, 0], raw.path[0, 0, 1] = V, 3
        raw.row_base[0, 0] = 1
    elif where == "row":   # a row entry with var = n_vars
        raw.row_excl[0, 0, 0], raw.row_excl[0, 0, 1] = V, 3
    else:                  # a row_base beyond path_capacity
        raw.row_base[0, 0] = 17
    cn = raw.run(512)
    print("malformed", where, cn.tolist())
    assert cn[0, :4].tolist() == [1, 0, 0, 2] and int(raw.stop[0]) == 1 and int(raw.sp[0]) == 0
    assert tuple(cn[1, :3].tolist()) == ENUM_TREE[(6, "middle")] and cn[1, 3] == 0
    with pytest.raises(E.PcpError) as e:  # the sticky violation word; reading it reports and clears it
        ctx.stats_read()
    assert e.value.code == -2
    ctx.stats_read()


# ------------------------------------------------------------------------------------------------ 11. the refusals of the C entry
def test_abi_refusals(ctx):
    import torch
    import pcp_amd.engine as E
    import small_forest_cases as C
    import form_forest_cases as FC

    def split_still_runs():
        l8, u8 = NC.push(ctx, 8)
        r = ctx.dfs_forest(l8[None], u8[None], steps_per_launch=64, capacity=64)
        assert r["error"] == 0 and counts(r) == QUEENS8_SPLIT
        return l8, u8

    def refused(rc, code, *words):
        msg = ctx._L.pcp_last_error(ctx._h).decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)
        split_still_runs()

    lb0, ub0 = split_still_runs()
    raw = Raw(ctx, lb0, ub0, capacity=16)
    assert raw.call(0) == 0 and int(raw.counters[0, 0]) == 0 and int(raw.sp[0]) == 1  # n_steps = 0: PCP_OK, nothing is launched
    # PCP_ERR_ARG
    refused(raw.call(4, ex=False), -1, "null state / exclusions")
    refused(raw.call(4, st=False), -1, "null state / exclusions")
    refused(raw.call(4, ex_over={"val": 2}), -1, "val")
    refused(raw.call(4, ex_over={"row_base": None}), -1, "row_base")
    refused(raw.call(4, ex_over={"row_excl": None}), -1, "row_excl")
    refused(raw.call(4, ex_over={"path": None}), -1, "path")  # path_capacity > 0 and no path
    refused(raw.call(4, st_over={"capacity": 1}), -1, "capacity < 2")
    raw.T = 0
    refused(raw.call(4), -1, "no tree")
    raw.T = 1
    props = M.lower_units([M.XNeqY(M.Identity(0), M.Identity(1))], 2)
    ctx.set_model(2, props, set_words=1)
    ctx.set_hull(0, 5)
    refused(Raw(ctx, np.zeros(2, np.int32), np.full(2, 5, np.int32), capacity=16).call(4), -1, "interval-mode", "pcp_dfs_forest_device_set_enum")
    # PCP_ERR_UNSUPPORTED
    vs, cs, _ = C.golomb(5)
    M.push_model(ctx, cs, len(vs))
    gl, gu = vs.bounds()
    refused(Raw(ctx, gl, gu, capacity=16).call(4), -5, "all-XNeqY", "pcp_dfs_forest_device_small_enum")
    vs, cs, _ = FC.schedule("A4")
    M.push_model(ctx, cs, len(vs))
    sl, su = vs.bounds()
    refused(Raw(ctx, sl, su, capacity=16).call(4), -5, "all-XNeqY", "pcp_dfs_forest_device_form_enum")
    NC.push(ctx, 8)
    raw = Raw(ctx, lb0, ub0, capacity=16)
    ctx.set_option("implicit_active", 0)
    try:
        rc = raw.call(4)
    finally:
        ctx.set_option("implicit_active", 1)
    refused(rc, -5, "explicit-active")
    best = torch.full((1,), E.no_incumbent("min"), dtype=torch.int32, device=raw.dev)
    raw.obj = E.ForestObjective(0, 0, best.data_ptr(), best.data_ptr(), None)
    refused(raw.call(4), -5, "branch and bound", "pcp_dfs_forest_device_small_enum")
    raw.obj = None
    sink = E.SolutionSink(8, len(lb0), raw.dev)
    ctx.solution_sink_set(sink)
    try:
        rc = raw.call(4)
        msg = ctx._L.pcp_last_error(ctx._h).decode()
    finally:
        ctx.solution_sink_set(None)
    assert rc == -5 and "sink" in msg
    split_still_runs()
    with E.var_select_scope(ctx, "input_order"):
        rc = raw.call(4)
        msg = ctx._L.pcp_last_error(ctx._h).decode()
    assert rc == -5 and "PCP_VAR_INPUT_ORDER" in msg
    split_still_runs()
    # nothing was launched by any of them: the tree is where it was, and runs
    assert int(raw.counters[0, 0]) == 0 and int(raw.sp[0]) == 1
    cn = raw.run(64)[0]
    assert tuple(cn[:3].tolist()) == ENUM_TREE[(8, "middle")] and cn[3] == 0
    # the drivers refuse the same before the entry is reached
    with pytest.raises(ValueError):
        ctx.dfs_forest_enum(lb0[None], ub0[None], forest="neq", objective=(0, "min"))
    with pytest.raises(ValueError):
        ctx.dfs_forest_enum(lb0[None], ub0[None], forest="neq", var_select="input_order")
