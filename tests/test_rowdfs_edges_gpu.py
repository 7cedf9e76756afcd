"""The terminal conditions of the row-stack search loop of the Interval forests (pcp_rowdfs.hpp: formdfs_kernel<BNB, SINK>,
smalldfs_kernel<BNB, ENUM, SINK>), ONE table over every instantiation that can reach each of them, so that a condition is pinned on both
kernels and not on the one it was first written for.  Two stores of four and five variables on domains of six and five values; 3 and 5
trees, so that a 256-thread workgroup has a wavefront without a tree (and, under branch and bound, wavefronts whose tree has finished:
only tree 0 is live there, one incumbent shared by several live trees makes their counters depend on timing); stacks of 2 - 4 rows.

Expected values never come from a forest kernel: BinarySplit from Context.dfs_device (dfs_step_kernel, the stated specification), stepped
with the same number of steps; Enumerate and branch and bound from the host-stepped searches pcp_amd.search.dfs / dfs_enumerate.  Only
the seam row also compares the forest with itself (n_steps = 1 repeated against one launch), which is what a seam is.

Rows other files assert already, not repeated here:
  error 2 from a popped bound, plain form / small:         test_form_forest_gpu / test_small_forest_gpu::test_edge_roots_in_one_launch
  error 2 from row_excl.var and a path entry >= n_vars:    test_small_enum_forest_gpu::test_a_malformed_entry_stops_its_tree_alone (plain ENUM)
  error 5, plain ENUM:                                     test_small_enum_forest_gpu::test_error_5_leaves_the_row_alone
  the StopNode limit, plain form / small and every SINK:   test_*_forest_gpu::test_one_tree_leaves_what_dfs_device_leaves,
                                                           test_forest_sink_gpu::test_the_limit_node_is_counted_and_not_appended
  a fold that empties a node is a node and a failed node:  the one-tree-against-the-host tests of test_form_forest_gpu, test_small_forest_gpu,
                                                           test_small_enum_forest_gpu, test_bnb_forest_gpu (their counters are the host's)
Error 3 (Unknown, every variable fixed) is left out: a unit that is not entailed on fixed domains does not exist among the propagators
the public API can push — on points every one of them is True or False."""
import ctypes as C_
import functools

import numpy as np
import pytest

from pcp_amd import model as M
from pcp_amd import search as S

pytestmark = pytest.mark.gpu

# (store, brancher, val, branch and bound, sink): the nine instantiations, Enumerate under both selectors
INSTS = [("form", "split", "middle", False, False), ("form", "split", "middle", True, False), ("form", "split", "middle", False, True),
         ("small", "split", "middle", False, False), ("small", "split", "middle", True, False), ("small", "split", "middle", False, True),
         ("small", "enum", "middle", False, False), ("small", "enum", "min", False, False), ("small", "enum", "middle", True, False),
         ("small", "enum", "middle", False, True)]
ENUMS = [i for i in INSTS if i[1] == "enum"]


def iid(i):
    return "-".join([i[0], i[1], i[2]] + (["bnb"] if i[3] else []) + (["sink"] if i[4] else []))


@functools.lru_cache(maxsize=None)
def build(store):
    """small: five queens and q0 < q4 (not all-XNeqY: pcp_dfs_device steps it), domains 1..5.  form: three tasks of length 2 on 0..5 that
    never overlap — a Disjunction per pair — and a fourth variable below the first; domains of six values.  (vs, cs, objective variable)."""
    if store == "small":
        vs, cs = M.nqueens(5)
        cs.alloc(M.XLessY(M.Identity(0), M.Identity(4)))
        return vs, cs, 0
    vs, cs = M.VStore(), M.CStore()
    x = [vs.alloc((0, 5)) for _ in range(3)]
    y = vs.alloc((0, 5))
    for i in range(3):
        for j in range(i + 1, 3):
            cs.alloc(M.Or((M.XLessY(M.Addition(x[i], 1), x[j]), M.XLessY(M.Addition(x[j], 1), x[i]))))
    cs.alloc(M.XLessY(y, x[0]))
    return vs, cs, 3


def roots(store, trees, fixed=True):
    """Tree t: the root with variable 1 fixed to its t-th value; fixed = False: the root itself, `trees` times."""
    vs, _, _ = build(store)
    lb0, ub0 = vs.bounds()
    L, U = np.repeat(lb0[None], trees, 0).astype(np.int32), np.repeat(ub0[None], trees, 0).astype(np.int32)
    if fixed:
        L[:, 1] = U[:, 1] = lb0[1] + np.arange(trees)
    return L, U


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


def push(ctx, store):
    vs, cs, var = build(store)
    M.push_model(ctx, cs, len(vs))
    return var


class Raw:
    """T trees on given roots and the C entry of the instantiation, one call per launch.  live: the trees that start with a row (branch
    and bound: tree 0 alone)."""

    def __init__(self, ctx, inst, L, U, capacity, path_capacity=8, sink_rows=256):
        import torch
        import pcp_amd.engine as E
        self.E, self.ctx, self.torch, self.inst = E, ctx, torch, inst
        store, brancher, val, bnb, sink = inst
        self.dev = dev = torch.device("cuda", ctx.device)
        self.T, self.V = L.shape
        self.var = push(ctx, store)
        z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device=dev)
        self.z = z
        self.sp, self.stop, self.counters = torch.ones(self.T, dtype=torch.int32, device=dev), z(self.T), z(self.T, 5, dt=torch.int64)
        if bnb:
            self.sp[1:] = 0
            none = E.no_incumbent("min")
            self.best, self.tree_best = torch.full((1,), none, dtype=torch.int32, device=dev), torch.full((self.T,), none, dtype=torch.int32, device=dev)
            self.tree_row = z(self.T, self.V)
            self.obj = E.ForestObjective(self.var, E.OBJ_MODES["min"], self.best.data_ptr(), self.tree_best.data_ptr(), self.tree_row.data_ptr())
        self.cap = 0
        self.grow(capacity, L, U)
        self.path_capacity = 0
        self.set_path(path_capacity)
        if sink:
            self.s_lb, self.s_ub, self.s_tree, self.s_count = z(sink_rows, self.V), z(sink_rows, self.V), z(sink_rows), z(1)
            self.sink_rows = sink_rows
            self.attach()

    def attach(self):
        """This Raw's sink becomes the context's (a context has one: the Raw built last took it)."""
        if self.inst[4]:
            s = self.E.PcpSolutionSink(self.s_lb.data_ptr(), self.s_ub.data_ptr(), self.s_tree.data_ptr(), self.s_count.data_ptr(), self.sink_rows, 0)
            assert self.ctx._L.pcp_solution_sink_set(self.ctx._h, C_.byref(s)) == 0

    def close(self):
        assert self.ctx._L.pcp_solution_sink_set(self.ctx._h, None) == 0

    def grow(self, capacity, L=None, U=None):
        """Stacks of `capacity` rows, the open rows kept; unused rows hold -77."""
        torch, old = self.torch, self.cap
        new = lambda *s: torch.full(s, -77, dtype=torch.int32, device=self.dev)
        lb, ub, base, excl = new(self.T, capacity, self.V), new(self.T, capacity, self.V), self.z(self.T, capacity), self.z(self.T, capacity, 2)
        excl[:, :, 0] = -1
        if old:
            lb[:, :old], ub[:, :old], base[:, :old], excl[:, :old] = self.lb, self.ub, self.row_base, self.row_excl
        else:
            lb[:, 0], ub[:, 0] = torch.from_numpy(L).to(self.dev), torch.from_numpy(U).to(self.dev)
        self.lb, self.ub, self.row_base, self.row_excl, self.cap = lb, ub, base, excl, capacity
        self.status = self.z(self.T, capacity, dt=torch.uint8)

    def set_path(self, path_capacity):
        old = getattr(self, "path", None)
        self.path = self.z(self.T, max(path_capacity, 1), 2)
        if old is not None:
            k = min(old.shape[1], self.path.shape[1])
            self.path[:, :k] = old[:, :k]
        self.path_capacity = path_capacity

    def resume(self):
        self.counters[:, 3] = 0
        self.stop.zero_()

    def call(self, n_steps, node_limit=0):
        E, L, h = self.E, self.ctx._L, self.ctx._h
        store, brancher, val, bnb, sink = self.inst
        st = E.DfsState(self.lb.data_ptr(), self.ub.data_ptr(), self.cap, self.sp.data_ptr(), self.stop.data_ptr(), self.status.data_ptr(), self.counters.data_ptr(),
                        None, None)
        obj = C_.byref(self.obj) if bnb else None
        if brancher == "enum":
            x = E.ForestExcl(self.path.data_ptr() if self.path_capacity else None, self.row_base.data_ptr(), self.row_excl.data_ptr(), self.path_capacity, E.VAL_MODES[val])
            rc = L.pcp_dfs_forest_device_small_enum(h, C_.byref(st), self.T, C_.byref(x), obj, n_steps, 0, node_limit, None)
        elif bnb:
            rc = (L.pcp_dfs_forest_device_form_bnb if store == "form" else L.pcp_dfs_forest_device_small_bnb)(h, C_.byref(st), self.T, obj, n_steps, node_limit, None)
        else:
            rc = (L.pcp_dfs_forest_device_form if store == "form" else L.pcp_dfs_forest_device_small)(h, C_.byref(st), self.T, n_steps, 0, node_limit, None)
        self.torch.cuda.synchronize()
        assert rc == 0
        assert self.ctx.last_plan()["path"] == (3 if store == "form" else 4) and self.ctx.last_plan()["grid"] == -(-self.T // 4)
        return rc

    def run(self, n_steps=64):
        for _ in range(1 << 12):
            self.call(n_steps)
            if not ((self.sp > 0) & (self.stop == 0)).any():
                break
        return self.counters.cpu().numpy()

    def state(self):
        """What a caller sees between two launches: sp, stop, the counters and every open row (ENUM: with its two words)."""
        sp, out = self.sp.cpu().tolist(), []
        cn, stop = self.counters.cpu().numpy(), self.stop.cpu().tolist()
        for t in range(self.T):
            rows = (self.lb[t, :sp[t]].cpu().numpy().tolist(), self.ub[t, :sp[t]].cpu().numpy().tolist())
            words = (self.row_base[t, :sp[t]].cpu().tolist(), self.row_excl[t, :sp[t]].cpu().tolist()) if self.inst[1] == "enum" else None
            out.append((sp[t], stop[t], cn[t].tolist(), rows, words))
        return out


def live_trees(inst, trees):
    return [0] if inst[3] else list(range(trees))


_SPEC = {}


def spec_steps(ctx, store, root, k, capacity):
    """dfs_step_kernel after k steps from that root on a stack of `capacity` rows: (sp, stop, [nodes, solutions, failed, error], lb rows, ub rows)."""
    key = (store, tuple(root[0].tolist()), tuple(root[1].tolist()), k, capacity)
    if key not in _SPEC:
        push(ctx, store)
        info = {}
        r = ctx.dfs_device(root[0], root[1], k, capacity=capacity, stop_on_solution=False, chunk=k, info=info)
        assert ctx.last_plan()["path"] != 1  # (the stepping path, not the all-XNeqY search loop)
        _SPEC[key] = (r["open"], int(r["stopped"]), [r["nodes"], r["solutions"], r["failed"], r["error"]], info["rows"][0].tolist(), info["rows"][1].tolist())
    return _SPEC[key]


def totals(ctx, inst, root):
    """(nodes, solutions, failed, best) of the complete tree below that root by the host-stepped search of the instantiation's brancher."""
    store, brancher, val, bnb, _ = inst
    key = ("totals", store, brancher, val, bnb, tuple(root[0].tolist()), tuple(root[1].tolist()))
    if key not in _SPEC:
        var = push(ctx, store)
        kw = dict(objective=(var, "min")) if bnb else dict(all_solutions=True)
        st = S.dfs(ctx, root[0], root[1], batch=1, **kw) if brancher == "split" else S.dfs_enumerate(ctx, root[0], root[1], batch=1, val=val, **kw)
        _SPEC[key] = (st.num_nodes, st.num_solution, st.num_failed_node, st.best)
    return _SPEC[key]


def first_solution_at(ctx, inst, root):
    """(k, failed before it): the first solution of the tree is its node k (the same with and without an objective: no incumbent yet)."""
    store, brancher, val, _, _ = inst
    push(ctx, store)
    st = S.dfs(ctx, root[0], root[1], batch=1) if brancher == "split" else S.dfs_enumerate(ctx, root[0], root[1], batch=1, val=val)
    assert st.num_solution == 1
    return st.num_nodes, st.num_failed_node


def check_done(ctx, raw, L, U, trees=None):
    """Every live tree ran to the end of its subtree: the host's totals, no error, nothing open."""
    cn = raw.counters.cpu().numpy()
    for t in live_trees(raw.inst, raw.T) if trees is None else trees:
        want = totals(ctx, raw.inst, (L[t], U[t]))
        assert tuple(cn[t, :3].tolist()) == want[:3] and cn[t, 3] == 0 and int(raw.sp[t]) == 0, (t, cn[t].tolist(), want)
        if raw.inst[3]:
            assert int(raw.best[0]) == want[3] == int(raw.tree_best[t]) and int(raw.tree_row[t, raw.var]) == want[3]


def violation_was_raised(ctx):
    import pcp_amd.engine as E
    with pytest.raises(E.PcpError) as e:  # the sticky word; reading it reports and clears it
        ctx.stats_read()
    ctx.stats_read()
    return e.value.code == -2


# ------------------------------------------------------------------------------------------------ error 1: the stack is full
@pytest.mark.parametrize("trees", [3, 5])
@pytest.mark.parametrize("inst", INSTS, ids=iid)
def test_error_1_keeps_the_node_propagated_and_uncounted(ctx, inst, trees):
    L, U = roots(inst[0], trees, fixed=False)  # (below a fixed variable two rows are enough for some subtrees)
    raw = Raw(ctx, inst, L, U, capacity=2)
    try:
        raw.call(64)
        cn, hit = raw.counters.cpu().numpy(), []
        for t in live_trees(inst, trees):
            if cn[t, 3] == 0:  # (a root that fails or is a solution at once, or whose subtree fits two rows)
                continue
            hit.append(t)
            assert cn[t, 3] == 1 and int(raw.stop[t]) == 1 and int(raw.sp[t]) == 2, (t, cn[t].tolist())
            top = (raw.lb[t, 1].cpu().numpy(), raw.ub[t, 1].cpu().numpy())
            lb, ub, _, st, _ = ctx.propagate(top[0][None], top[1][None])  # propagated: the row is a fixpoint of the store, and not a failed one
            assert st[0] != M.FALSE and np.array_equal(lb[0], top[0]) and np.array_equal(ub[0], top[1]), t
            if inst[1] == "enum":  # its list is in the path already: it inherits, and appends nothing
                assert raw.row_excl[t, 1].cpu().tolist() == [-1, 0] and 0 <= int(raw.row_base[t, 1]) <= raw.path_capacity
            if inst[1] == "split" and not inst[3]:  # uncounted: the counters and rows of dfs_step_kernel on two rows
                sp, stop, c4, rl, ru = spec_steps(ctx, inst[0], (L[t], U[t]), 64, 2)
                assert (sp, stop, c4) == (2, 1, cn[t, :4].tolist()) and raw.lb[t, :2].cpu().tolist() == rl and raw.ub[t, :2].cpu().tolist() == ru, t
        assert hit, "no tree filled a stack of two rows"
        raw.grow(16)  # resumed with a larger stack: the totals of a run whose stack never fills
        raw.resume()
        raw.run()
        check_done(ctx, raw, L, U)
    finally:
        raw.close()


# ------------------------------------------------------------------------------------------------ sp > capacity on entry
@pytest.mark.parametrize("trees", [3, 5])
@pytest.mark.parametrize("inst", INSTS, ids=iid)
def test_a_stack_pointer_beyond_the_rows_touches_nothing(ctx, inst, trees):
    L, U = roots(inst[0], trees)
    raw = Raw(ctx, inst, L, U, capacity=16)
    try:
        bad = 1
        raw.sp[bad] = 17
        before = (raw.lb[bad].clone(), raw.ub[bad].clone(), raw.row_base[bad].clone(), raw.row_excl[bad].clone(), raw.path[bad].clone())
        raw.run()
        assert raw.counters[bad].cpu().tolist() == [0, 0, 0, 1, 0] and int(raw.stop[bad]) == 1 and int(raw.sp[bad]) == 17
        after = (raw.lb[bad], raw.ub[bad], raw.row_base[bad], raw.row_excl[bad], raw.path[bad])
        assert all(bool((a == b).all()) for a, b in zip(before, after))
        # ... and the trees next to it run as if it were not there
        others = [t for t in live_trees(inst, trees) if t != bad]
        check_done(ctx, raw, L, U, trees=others)
        if inst[4]:
            assert int(raw.s_count[0]) == sum(totals(ctx, inst, (L[t], U[t]))[1] for t in others)
    finally:
        raw.close()


# ------------------------------------------------------------------------------------------------ error 2: refused, not wrapped
# (the plain ENUM instantiation under row_excl: test_small_enum_forest_gpu; a BinarySplit row has no exclusion words)
ERROR_2 = [(i, "bound") for i in INSTS if i[1] == "enum" or i[3] or i[4]] + [(i, "row_base") for i in ENUMS] + [(i, "row_excl") for i in ENUMS if i[3] or i[4]]


@pytest.mark.parametrize("inst,how", ERROR_2, ids=lambda p: iid(p) if isinstance(p, tuple) else p)
def test_error_2_counts_pops_and_stops(ctx, inst, how):
    L, U = roots(inst[0], 3)
    ctx.stats_read()
    raw = Raw(ctx, inst, L, U, capacity=16, path_capacity=2)
    try:
        bad = 0  # (the live tree of branch and bound)
        if how == "bound":
            raw.ub[bad, 0, 2] = raw.E.BOUND_MAX + 1
        elif how == "row_base":
            raw.row_base[bad, 0] = 3  # > path_capacity
        else:
            raw.row_excl[bad, 0, 0], raw.row_excl[bad, 0, 1] = raw.V, 2
        raw.run()
        assert raw.counters[bad, :4].cpu().tolist() == [1, 0, 0, 2] and int(raw.stop[bad]) == 1 and int(raw.sp[bad]) == 0
        assert violation_was_raised(ctx)
        if inst[3]:
            assert int(raw.best[0]) == raw.E.no_incumbent("min")
        else:
            check_done(ctx, raw, L, U, trees=[1, 2])  # it stops alone
        if inst[4]:
            assert int(raw.s_count[0]) == sum(totals(ctx, inst, (L[t], U[t]))[1] for t in (1, 2))
    finally:
        raw.close()


# ------------------------------------------------------------------------------------------------ error 5: the path is full
@pytest.mark.parametrize("inst", [i for i in ENUMS if i[3] or i[4]], ids=iid)
def test_error_5_changes_nothing(ctx, inst):
    """The root arrives with an entry of its own and a path of no entries.  (The entry's value lies above the domain: entailed, so the tree
    below is the root's own, which the host search gives.)"""
    L, U = roots(inst[0], 3)
    raw = Raw(ctx, inst, L, U, capacity=16, path_capacity=0)
    try:
        for t in range(3):
            raw.row_excl[t, 0, 0], raw.row_excl[t, 0, 1] = 2, int(U[t, 2]) + 1
        raw.call(64)
        for t in live_trees(inst, 3):
            assert raw.counters[t].cpu().tolist() == [0, 0, 0, 5, 0] and int(raw.stop[t]) == 1 and int(raw.sp[t]) == 1, t
            assert np.array_equal(raw.lb[t, 0].cpu().numpy(), L[t]) and np.array_equal(raw.ub[t, 0].cpu().numpy(), U[t])
            assert raw.row_excl[t, 0].cpu().tolist() == [2, int(U[t, 2]) + 1] and int(raw.row_base[t, 0]) == 0
        if inst[4]:
            assert int(raw.s_count[0]) == 0
        raw.set_path(8)  # resumed with a larger path: the totals of a run whose path never fills
        raw.resume()
        raw.run()
        check_done(ctx, raw, L, U)
    finally:
        raw.close()


# ------------------------------------------------------------------------------------------------ the StopNode limit
@pytest.mark.parametrize("inst", [i for i in INSTS if not i[4] and (i[1] == "enum" or i[3])], ids=iid)
def test_the_limit_node_is_a_node_and_nothing_else(ctx, inst):
    vs, _, _ = build(inst[0])
    lb0, ub0 = (np.ascontiguousarray(a, np.int32) for a in vs.bounds())
    k, failed = first_solution_at(ctx, inst, (lb0, ub0))
    assert k > 2
    L, U = np.repeat(lb0[None], 3, 0), np.repeat(ub0[None], 3, 0)
    for limit, want in ((k, [k, 0, failed, 0]), (k + 1, None)):
        raw = Raw(ctx, inst, L, U, capacity=16)
        try:
            for _ in range(k + 2):
                raw.call(3, node_limit=limit)
            for t in live_trees(inst, 3):
                cn = raw.counters[t, :4].cpu().tolist()
                assert int(raw.stop[t]) == 1 and cn[0] == limit and cn[3] == 0, (t, cn)
                if want:  # the solution is the limit node: counted as a node, neither a solution nor a failure, no incumbent
                    assert cn == want and (not inst[3] or int(raw.tree_best[t]) == raw.E.no_incumbent("min"))
                else:  # one node later: the solution is one, and the node after it is the limit node
                    assert cn == [k + 1, 1, failed, 0] and (not inst[3] or int(raw.tree_best[t]) == int(raw.tree_row[t, raw.var]) == int(raw.best[0]))
        finally:
            raw.close()


# ------------------------------------------------------------------------------------------------ launch seams
@pytest.mark.parametrize("trees", [3, 5])
@pytest.mark.parametrize("inst", INSTS, ids=iid)
def test_launch_seams(ctx, inst, trees):
    """n_steps = 1 repeated against one launch of k steps, k = 1 .. 14, on stacks of four rows (some trees fill them: error 1 is a seam too):
    equal sp, open rows — the persisted left child, and under ENUM its two words —, counters and stop; BinarySplit without an objective
    also against dfs_step_kernel after k steps."""
    L, U = roots(inst[0], trees)
    one = Raw(ctx, inst, L, U, capacity=4)
    try:
        for k in range(1, 15):
            one.call(1)
            many = Raw(ctx, inst, L, U, capacity=4)
            many.call(k)
            one.attach()
            a, b = one.state(), many.state()
            assert a == b, (k, a, b)
            if inst[4]:
                assert int(one.s_count[0]) == sum(s[2][1] for s in a)
            if inst[1] == "split" and not inst[3]:
                for t in range(trees):
                    sp, stop, c4, rl, ru = spec_steps(ctx, inst[0], (L[t], U[t]), k, 4)
                    assert (a[t][0], a[t][1], a[t][2][:4], a[t][3]) == (sp, stop, c4, (rl, ru)), (k, t)
    finally:
        one.close()


# ------------------------------------------------------------------------------------------------ branch and bound: each tree's last solution
@pytest.mark.parametrize("inst", [i for i in INSTS if i[3]], ids=iid)
def test_every_tree_keeps_its_last_solution(ctx, inst):
    """Three live trees under one incumbent (their counters depend on timing, these do not): a tree that found a solution keeps its value
    and its row — a solution of the store whose objective is that value —, the best of them is the incumbent, and the incumbent is the
    optimum over the three subtrees by the host search."""
    L, U = roots(inst[0], 3)
    raw = Raw(ctx, inst, L, U, capacity=16)
    try:
        raw.sp[:] = 1
        raw.run(5)
        none = raw.E.no_incumbent("min")
        tb, rows = raw.tree_best.cpu().tolist(), raw.tree_row.cpu().numpy()
        found = [t for t in range(3) if tb[t] != none]
        best = [totals(ctx, inst, (L[t], U[t]))[3] for t in range(3)]
        assert found and int(raw.best[0]) == min(tb) == min(b for b in best if b is not None)
        assert (raw.counters[:, 3] == 0).all() and (raw.sp == 0).all()
        push(ctx, inst[0])
        for t in found:
            assert int(rows[t, raw.var]) == tb[t] and (L[t] <= rows[t]).all() and (rows[t] <= U[t]).all(), t
            _, _, _, st, _ = ctx.propagate(rows[t][None], rows[t][None])
            assert st[0] == M.TRUE, t
            assert int(raw.counters[t, 1]) >= 1
        for t in range(3):
            assert (tb[t] == none) == (int(raw.counters[t, 1]) == 0), t
    finally:
        raw.close()
