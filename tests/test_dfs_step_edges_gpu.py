"""The stepping path of pcp_dfs_device (one fixpoint launch of the generic kernels, then dfs_step_kernel, per node) at its edges: more
variables than the 256 threads of the step kernel, a stack that is too small by every amount down to the capacity at which it stops being
too small, and a root the engine refuses.  The models are not all-XNeqY, so the in-kernel search loop never takes them; every test asserts
from last_plan() that the generic kernels ran.  The reference is OracleModel.search: its counters, its first solution, and its tree — the
stack row of every node is read off the recorded statuses.  Integer work, no tolerance."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from pcp_amd import model as M
import pcp_amd.engine as E

import branch_cases as B

pytestmark = pytest.mark.gpu

DEFAULTS = {"force_path": 0, "nodes_per_block": 0, "block_threads": 1024, "team": 0, "list_cap": 2048, "global_dom": 0, "packed": 1, "word_level": 1,
            "neq_dfs": 1, "small_path": 1}
AMPLE = 64  # a stack no search of this file fills


@pytest.fixture(scope="module")
def ctx():
    c = E.Context(0)
    yield c
    c.close()


def stepping(ctx, **opts):
    """The options under which pcp_dfs_device steps: no in-kernel search loop, no small-store kernel."""
    for k, v in {**DEFAULTS, "neq_dfs": 0, "small_path": 0, **opts}.items():
        ctx.set_option(k, v)


def restore(ctx):
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)


def _props(rows):
    props = np.zeros(len(rows), dtype=M.PROP_DTYPE)
    props["var"][:] = M.PCP_NOVAR
    props["group"] = np.arange(len(rows))
    for r, (kind, x, y, c) in enumerate(rows):
        props[r]["kind"] = kind
        props[r]["var"][0], props[r]["var"][1], props[r]["off"][1] = x, y, c
    return props


def walk(status):
    """The stack of dfs_step_kernel over a tree given as the statuses of its nodes in the order the search visits them.  The root is row 0
    (sp = 1); an Unknown node in row sp - 1 needs sp < capacity, leaves its right child in its row and puts the left one on top.  Returns
    (sp of every node, the sp of the rows still open at the end, the least capacity that never overflows)."""
    pending, sps, need = [1], [], 2
    for st in status:
        sp = pending.pop()
        sps.append(sp)
        if st == M.UNKNOWN:
            need = max(need, sp + 1)
            pending += [sp, sp + 1]  # the right child waits in the parent's row, the left one is taken next
    return sps, pending, need


# ---------------------------------------------------------------------------------------------------------------- wide V
WIDE = {257: 102, 300: 104}  # V: seed
N_FREE = 24


@functools.lru_cache(maxsize=None)
def wide_model(V):
    """V variables, all but 24 assigned at the root; the free ones — 1, 63, 64, 70, 255, 256 and V - 1 among them — in all-different
    triples (`x != y`) over three or four values, tied by `x < y + c` and `x != y + c`; V more records over the assigned ones.
    Domains inside [0, 12]."""
    rng = np.random.default_rng(WIDE[V])
    must = [1, 63, 64, 70, 255, 256, V - 1]
    rest = rng.choice(np.setdiff1d(np.arange(V), must), size=N_FREE - len(must), replace=False)
    free = rng.permutation(np.concatenate([must, rest]))
    val = rng.integers(0, 13, size=V)
    lb, ub = val.astype(np.int32), val.astype(np.int32)
    rows = []
    for g in (free[i:i + 3] for i in range(0, N_FREE, 3)):
        a, w = int(rng.integers(0, 10)), int(rng.integers(2, 4))
        for x in g:
            lb[x], ub[x] = a, min(12, a + w)
        rows += [(M.NEQ, g[i], g[j], 0) for i in range(len(g)) for j in range(i + 1, len(g))]
    for _ in range(N_FREE // 2):
        x, y = rng.choice(free, size=2, replace=False)
        if rng.random() < 0.5:
            rows.append((M.LT, x, y, int(lb[x]) - int(lb[y]) + int(rng.integers(1, 4))))
        else:
            rows.append((M.NEQ, x, y, int(lb[x]) - int(lb[y]) + int(rng.integers(-1, 2))))
    for _ in range(V):
        x, y = rng.choice(V, size=2, replace=False)
        if rng.random() < 0.5:
            rows.append((M.LT, x, y, int(ub[x]) - int(lb[y]) + 1 + int(rng.integers(0, 3))))  # holds whatever the two take
        else:
            rows.append((M.NEQ, x, y, int(lb[x]) - int(lb[y]) + int(rng.choice([-2, -1, 1, 2]))))
    return _props(rows), lb, ub


@functools.lru_cache(maxsize=None)
def wide_reference(V, all_solutions):
    props, lb, ub = wide_model(V)
    ss, _, rec, first = orc.OracleModel(V, props).search(lb, ub, all_solutions=all_solutions, node_limit=150 if all_solutions else 0, max_records=400)
    assert len(rec["status"]) == ss["num_nodes"]
    _, pending, need = walk(rec["status"])
    branched = [B.ref_var(l, u) for l, u, st in zip(rec["lb_out"], rec["ub_out"], rec["status"]) if st == M.UNKNOWN]
    return ss, first, len(pending), need, branched


@pytest.mark.parametrize("chunk", [1, 7, 97])
@pytest.mark.parametrize("V", list(WIDE))
def test_more_variables_than_threads(ctx, V, chunk):
    """V = 257 and 300: threads of the step kernel's 256 take a second variable; variables on both sides of index 256 are branched on."""
    props, lb0, ub0 = wide_model(V)
    assert {int(k) for k in set(props["kind"].tolist())} == {M.NEQ, M.LT} and int(lb0.min()) >= 0 and int(ub0.max()) <= 12
    ctx.set_model(V, props)
    stepping(ctx)
    try:
        # the first solution
        ss, first, n_open, need, branched = wide_reference(V, False)
        assert ss["num_solution"] == 1 and ss["num_failed_node"] >= 1 and need <= AMPLE and ss["num_nodes"] < 400
        assert any(v >= 256 for v in branched) and any(v < 256 for v in branched)
        r = ctx.dfs_device(lb0, ub0, 400, capacity=AMPLE, stop_on_solution=True, chunk=chunk)
        plan = ctx.last_plan()
        assert plan["path"] == 0 and plan["implicit_active"] == 1, plan
        got = (r["nodes"], r["solutions"], r["failed"], r["error"], r["open"])
        assert got == (ss["num_nodes"], 1, ss["num_failed_node"], 0, n_open), (got, ss, n_open)
        assert r["stopped"] and np.array_equal(r["first_solution"], first)
        # every solution, under StopNode(150): the node that reaches the limit is a node and nothing else; its children stay open
        ss, first, n_open, need, branched = wide_reference(V, True)
        assert ss["num_nodes"] == 150 and ss["num_solution"] >= 1 and ss["num_failed_node"] >= 1 and need <= AMPLE
        assert any(v >= 256 for v in branched) and any(v < 256 for v in branched)
        r = ctx.dfs_device(lb0, ub0, 400, capacity=AMPLE, stop_on_solution=False, node_limit=150, chunk=chunk)
        assert ctx.last_plan()["path"] == 0
        got = (r["nodes"], r["solutions"], r["failed"], r["error"], r["open"])
        assert got == (150, ss["num_solution"], ss["num_failed_node"], 0, n_open), (got, ss, n_open)
        assert r["stopped"] and np.array_equal(r["first_solution"], first)
    finally:
        restore(ctx)


# ---------------------------------------------------------------------------------------------------------------- the stack
SMALL_V, SMALL_HI, SMALL_SEED = 5, 4, 4


@functools.lru_cache(maxsize=None)
def small_model():
    """Five all-different variables on [0, 4] with two `x < y + c`: a tree of about a hundred nodes, failures and solutions in it."""
    rng = np.random.default_rng(SMALL_SEED)
    rows = [(M.NEQ, x, y, 0) for x in range(SMALL_V) for y in range(x + 1, SMALL_V)]
    for _ in range(SMALL_V // 2):
        x, y = rng.choice(SMALL_V, size=2, replace=False)
        rows.append((M.LT, x, y, int(rng.integers(0, 3))))
    return _props(rows), np.zeros(SMALL_V, np.int32), np.full(SMALL_V, SMALL_HI, np.int32)


@functools.lru_cache(maxsize=None)
def small_reference():
    props, lb, ub = small_model()
    ss, _, rec, _ = orc.OracleModel(SMALL_V, props).search(lb, ub, all_solutions=True, max_records=1000)
    assert len(rec["status"]) == ss["num_nodes"] < 1000
    sps, pending, need = walk(rec["status"])
    assert not pending
    return ss, rec["status"], sps, need


def test_stack_overflow_down_to_the_capacity_that_suffices(ctx):
    """Every capacity from 2 to c* + 1, c* the capacity the deepest path of the oracle's tree needs.  Below c*: error 1 at the first Unknown
    node whose left child has no row — it stays on the stack, uncounted, so searching every open row as a root of its own and adding the
    counters gives the oracle's totals.  At c* and above: no error, the oracle's totals."""
    props, lb0, ub0 = small_model()
    ss, status, sps, c_star = small_reference()
    want = (ss["num_nodes"], ss["num_solution"], ss["num_failed_node"])
    assert 5 <= c_star <= 12 and 50 <= want[0] <= 200 and want[1] >= 1 and want[2] >= 1, (c_star, want)
    ctx.set_model(SMALL_V, props)
    stepping(ctx)
    try:
        for cap in range(2, c_star + 2):
            info = {}
            r = ctx.dfs_device(lb0, ub0, 2000, capacity=cap, stop_on_solution=False, chunk=97, info=info)
            assert ctx.last_plan()["path"] == 0
            got = (r["nodes"], r["solutions"], r["failed"])
            if cap >= c_star:
                assert r["error"] == 0 and r["open"] == 0 and not r["stopped"] and got == want, (cap, r)
                continue
            assert r["error"] == 1 and r["stopped"] and r["open"] > 0, (cap, r)
            # where it stops, from the oracle's tree: the first Unknown node in row cap - 1
            at = next(i for i, (st, sp) in enumerate(zip(status, sps)) if st == M.UNKNOWN and sp + 1 > cap)
            assert (r["nodes"], r["open"]) == (at, sps[at]), (cap, r, at, sps[at])
            assert r["solutions"] == int((status[:at] == M.TRUE).sum()) and r["failed"] == int((status[:at] == M.FALSE).sum())
            L, U = info["rows"]
            assert L.shape == (r["open"], SMALL_V)
            total = np.array(got)
            for row in range(r["open"]):
                sub = ctx.dfs_device(L[row], U[row], 2000, capacity=AMPLE, stop_on_solution=False, chunk=97)
                assert sub["error"] == 0 and sub["open"] == 0, (cap, row, sub)
                total += (sub["nodes"], sub["solutions"], sub["failed"])
            assert tuple(total.tolist()) == want, (cap, total, want)
    finally:
        restore(ctx)


def test_a_refused_root_ends_the_search_with_error_2(ctx):
    """A declared hull and a root below it, on the generic kernel that keeps a node as 10-bit cells counted from the hull's lower end (what
    those cells cannot hold is what this kernel refuses): the fixpoint launch refuses the row (PCP_STATUS_HULL), the step counts it, pops it
    and stops with error 2."""
    import torch
    props, lb0, ub0 = small_model()
    lb_bad = lb0.copy()
    lb_bad[2] = -1
    ctx.set_model(SMALL_V, props)
    ctx.set_hull(0, SMALL_HI)
    try:
        # pcp_dfs_device steps a model like this one under force_path 2: the same launch, on its own first
        stepping(ctx, global_dom=2, force_path=2)
        dev = torch.device("cuda", ctx.device)
        t_lb, t_ub = torch.from_numpy(lb_bad[None].copy()).to(dev), torch.from_numpy(ub0[None].copy()).to(dev)
        t_st = torch.zeros(1, dtype=torch.uint8, device=dev)
        ctx.stats_reset()
        ctx.propagate_device(1, t_lb, t_ub, t_lb, t_ub, None, None, t_st)
        torch.cuda.synchronize()
        assert ctx.last_plan()["path"] == 0 and t_st.cpu().tolist() == [B.HULL]
        assert np.array_equal(t_lb.cpu().numpy()[0], lb_bad) and np.array_equal(t_ub.cpu().numpy()[0], ub0)  # untouched
        with pytest.raises(E.PcpError) as ei:
            ctx.stats_read()
        assert ei.value.code == -2  # PCP_ERR_CONTRACT: the sticky flag, reported once
        ctx.stats_read()
        stepping(ctx, global_dom=2)
        r = ctx.dfs_device(lb_bad, ub0, 50, capacity=AMPLE, stop_on_solution=False, chunk=7)
        assert ctx.last_plan()["path"] == 0
        assert r["error"] == 2 and r["stopped"], r
        assert (r["nodes"], r["solutions"], r["failed"], r["open"]) == (1, 0, 0, 0), r
        with pytest.raises(E.PcpError):
            ctx.stats_read()
        ctx.stats_read()
        # the same root inside the hull, same options: the whole tree
        ss = small_reference()[0]
        ok = ctx.dfs_device(lb0, ub0, 2000, capacity=AMPLE, stop_on_solution=False, chunk=97)
        assert (ok["nodes"], ok["solutions"], ok["failed"], ok["error"], ok["open"]) == (ss["num_nodes"], ss["num_solution"], ss["num_failed_node"], 0, 0)
    finally:
        restore(ctx)
        ctx.set_model(SMALL_V, props)  # forgets the hull
