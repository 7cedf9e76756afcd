"""pcp_branch_device_excl — Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate> on the device, the brancher that writes exclusion
lists (pcp_enum.hip) — against pcp_amd.search.branch_enumerate, bit for bit: rows, offsets, entries, child_dirty and counts.  Then
DeviceSearch(brancher="enumerate"), the loop that keeps rows, hints and lists on the GPU, against search.dfs_enumerate."""
import numpy as np
import pytest

from pcp_amd import model as M
from pcp_amd import search as S
import pcp_amd.engine as E
from pcp_amd.search_device import DeviceSearch

pytestmark = pytest.mark.gpu

BIG = (1 << 29) - 1
HULL = 0xFE
JUNK = 3  # entries in front of the batch's lists: excl_off[0] != 0


@pytest.fixture(scope="module")
def ctxs():
    """One context per n_vars (the brancher reads nothing else of the model)."""
    made = {}

    def get(n_vars):
        if n_vars not in made:
            c = E.Context(0)
            c.set_model(n_vars, np.zeros(0, dtype=M.PROP_DTYPE))
            made[n_vars] = c
        return made[n_vars]
    yield get
    for c in made.values():
        c.close()


def _device(ctx, L, U, st, lists, val, reverse, capacity=None, dirty=True, null_off=False, shift=0):
    """Run the entry on a batch; lists[i] = node i's entries [(var, value)].  Returns the children and the counts as numpy arrays."""
    import torch
    dev = torch.device("cuda", 0)
    n, V = L.shape
    flat = np.array([(7, 7)] * JUNK + [tuple(p) for e in lists for p in e], np.int64).reshape(-1, 2).astype(np.int32)
    off = (JUNK + np.concatenate([[0], np.cumsum([len(e) for e in lists])])).astype(np.int32)
    m = sum(len(lists[i]) for i in range(n) if st[i] == 2)
    capacity = 2 * m + int((st == 2).sum()) if capacity is None else capacity

    def rows(a):  # (shift: the rows start `shift` int32 behind a 16-byte boundary)
        buf = torch.zeros(a.size + 8, dtype=torch.int32, device=dev)
        buf[shift:shift + a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
        return buf[shift:shift + a.size].view(a.shape)
    t_lb, t_ub = rows(L), rows(U)
    t_st = torch.from_numpy(st).to(dev)
    t_off, t_ex = torch.from_numpy(off).to(dev), torch.from_numpy(flat).to(dev)
    c_lb, c_ub = rows(np.full((2 * n, V), -77, np.int32)), rows(np.full((2 * n, V), -77, np.int32))
    c_dirty = torch.full((2 * n,), -7, dtype=torch.int32, device=dev) if dirty else None
    c_off = torch.full((2 * n + 1,), -7, dtype=torch.int32, device=dev)
    c_ex = torch.full((capacity + 4, 2), -7, dtype=torch.int32, device=dev)
    counts = torch.full((8,), -7, dtype=torch.int32, device=dev)
    ctx.set_option("branch_reverse", reverse)
    try:
        ctx.branch_device_excl(n, t_lb, t_ub, t_st, None if null_off else t_off, None if null_off else t_ex, val, c_lb, c_ub, c_off, c_ex, capacity, counts,
                               child_dirty=c_dirty)
        torch.cuda.synchronize()
    finally:
        ctx.set_option("branch_reverse", 0)
    # the inputs are never written
    assert np.array_equal(t_lb.cpu().numpy(), L) and np.array_equal(t_ub.cpu().numpy(), U) and np.array_equal(t_ex.cpu().numpy(), flat)
    assert (c_ex[capacity:].cpu().numpy() == -7).all()  # nothing behind the capacity
    return {"lb": c_lb.cpu().numpy(), "ub": c_ub.cpu().numpy(), "dirty": None if c_dirty is None else c_dirty.cpu().numpy(), "off": c_off.cpu().numpy(),
            "ex": c_ex.cpu().numpy(), "counts": counts.cpu().numpy()}


def _host(L, U, st, lists, val):
    """branch_enumerate on the Unknown rows (entries with var >= n_vars are dropped: nothing may use them as an index)."""
    V = L.shape[1]
    unk = np.nonzero(st == 2)[0]
    mine = [[p for p in lists[i] if 0 <= p[0] < V] for i in unk]
    poff = np.concatenate([[0], np.cumsum([len(e) for e in mine])]).astype(np.int64)
    pex = np.array([p for e in mine for p in e], np.int64).reshape(-1, 2).astype(np.int32)
    cl, cu, coff, cex, cd = S.branch_enumerate(L[unk], U[unk], poff, pex, val=val)
    return cl, cu, [cex[coff[c]:coff[c + 1]] for c in range(len(cl))], cd


def _compare(got, host, st, reverse, tag):
    cl, cu, rows, cd = host
    if reverse:
        cl, cu, rows, cd = cl[::-1], cu[::-1], rows[::-1], cd[::-1]
    k, total = len(cl), sum(len(r) for r in rows)
    want = [k, int((st == 1).sum()), int((st == 0).sum()), int((st == 2).sum()), int((st > 2).sum()), total, 0, 0]
    assert got["counts"].tolist() == want, (tag, got["counts"].tolist(), want)
    assert np.array_equal(got["lb"][:k], cl) and np.array_equal(got["ub"][:k], cu), tag
    assert (got["lb"][k:] == -77).all() and (got["ub"][k:] == -77).all(), tag
    assert got["off"][:k + 1].tolist() == np.concatenate([[0], np.cumsum([len(r) for r in rows])]).tolist(), tag
    flat = np.concatenate(rows).reshape(-1, 2) if k else np.zeros((0, 2), np.int32)
    assert np.array_equal(got["ex"][:total], flat), tag
    if got["dirty"] is not None:
        assert np.array_equal(got["dirty"][:k], cd), tag


DOMAINS = [(-3, -2), (-5, 4), (1, 2), (-BIG, BIG), (0, 9), (-40, 40)]  # truncation toward zero; a middle value that is a bound (both kinds) and folds


def _batch(V, n, k, seed):
    """n nodes over V variables with statuses mixed by position and lists of k entries built around each node's branching variable."""
    rng = np.random.default_rng(seed)
    dom = np.array(DOMAINS)[rng.integers(0, len(DOMAINS), size=(n, V))]
    L, U = dom[..., 0].astype(np.int32), dom[..., 1].astype(np.int32)
    fix = rng.random((n, V)) < 0.5  # assigned variables (never all of a row: variable i % V keeps its domain)
    fix[np.arange(n), np.arange(n) % V] = False
    L = np.where(fix, U, L).astype(np.int32)
    st = np.array([2, 2, 1, 2, 0, 2, HULL, 2], np.uint8)[np.arange(n) % 8]
    x = S.first_smallest_var(L, U)
    lists = []
    for i in range(n):
        lo, hi = int(L[i, x[i]]), int(U[i, x[i]])
        mid = int(S.middle_val(L[i:i + 1, x[i]], U[i:i + 1, x[i]])[0])
        free = hi if hi - lo > 1 else lo  # one value of x stays free (every value excluded is the error test's business)
        e = []
        for j in range(k):
            kind = int(rng.integers(0, 8))
            y = int(rng.integers(0, V))
            if kind == 0 and e:
                p = e[int(rng.integers(0, len(e)))]                    # a duplicate
            elif kind == 1:
                p = (y, int(U[i, y]) + 1 + int(rng.integers(0, 3)))     # outside the domain: dropped
            elif kind == 2:
                p = (y, int(L[i, y]) - 1)                              # outside, below
            elif kind == 3:
                p = (int(x[i]), min(max(mid + int(rng.integers(-3, 4)), lo), hi))  # on the branched variable, on both sides of v (and v itself)
            elif kind == 4:
                p = (int(x[i]), lo + 1 if lo + 1 <= hi else lo)        # exactly on the bound MinVal's fold leaves: kept
            elif kind == 5:
                p = (V + int(rng.integers(0, 3)), int(rng.integers(-5, 5)))  # var >= n_vars: dropped, never an index
            elif kind == 6:
                p = (y, int(rng.integers(int(L[i, y]), int(U[i, y]) + 1)) if U[i, y] - L[i, y] < 100 else int(rng.integers(-50, 50)))  # inside: kept
            else:
                p = (y, int(U[i, y]))                                  # on a bound of another variable: kept
            if p[0] == x[i] and p[1] == free:
                p = (p[0], lo if free == hi else hi)
            e.append((int(p[0]), int(p[1])))
        lists.append(e)
    return L, U, st, lists


@pytest.mark.parametrize("V", [1, 3, 4, 5, 63, 64, 65, 257])
def test_children_equal_branch_enumerate(ctxs, V):
    ctx = ctxs(V)
    for n in (1, 2, 65, 300):
        for k in (0, 1, 63, 64, 65, 300):
            L, U, st, lists = _batch(V, n, k, seed=1000 * V + 10 * n + k)
            for val in ("middle", "min"):
                host = _host(L, U, st, lists, val)
                for reverse in (0, 1):
                    # (the 65-node batches also with rows that start 4 bytes behind a 16-byte boundary)
                    got = _device(ctx, L, U, st, lists, val, reverse, shift=1 if n == 65 else 0)
                    _compare(got, host, st, reverse, (V, n, k, val, reverse))
    # no hints wanted; no lists given
    L, U, st, lists = _batch(V, 65, 5, seed=V)
    _compare(_device(ctx, L, U, st, lists, "middle", 1, dirty=False), _host(L, U, st, lists, "middle"), st, 1, (V, "dirty=NULL"))
    none = [[] for _ in lists]
    _compare(_device(ctx, L, U, st, none, "min", 0, null_off=True), _host(L, U, st, none, "min"), st, 0, (V, "excl_off=NULL"))


def test_a_value_already_excluded_is_not_chosen_again(ctxs):
    """v excluded, then chains of excluded neighbours: the free value only below, only above, at equal distance (the lower one wins), a domain
    narrower than the chain on one side, duplicates, and chains longer than one pass of the kernel's bitmaps."""
    V = 3
    ctx = ctxs(V)
    cases = []  # (lo, hi, values excluded on the branching variable)
    for c in (0, 1, 2, 5, 17, 40):
        below, above = list(range(-c, 0)), list(range(1, c + 1))
        cases += [(-100, 100, [0] + below + above),            # equal distance: v - d wins
                  (-100, 100, [0] + below + above + [-c - 1]),  # free only above at distance c + 1
                  (-100, 100, [0] + below + above + [c + 1]),   # free only below
                  (-100, 100, [0, 0] + above + above),          # duplicates; the nearest free value is just below
                  (10, 10 + 2 * c + 3, list(range(10, 10 + c + 1)))]  # MinVal's v = lb excluded with c neighbours above
    # a domain narrower than the chain on one side (v = 0 in both): the free value is the far bound of the other side
    cases += [(-3, 4, [0, -1, -2, -3, -4, -5, 1, 2, 3]), (-4, 3, [0, 1, 2, 3, 4, 5, -1, -2, -3])]
    cases += [(-5000, 5000, list(range(-2100, 2101))), (-5000, 5000, list(range(-2047, 2049))), (-BIG, BIG, [0, -1, 1, 2, -2, -3])]
    n = len(cases)
    L, U = np.full((n, V), 4, np.int32), np.full((n, V), 4, np.int32)
    L[:, 1], U[:, 1] = [c[0] for c in cases], [c[1] for c in cases]
    L[:, 2], U[:, 2] = -BIG, BIG  # (a wider variable: never the smallest, except in the last case, where the first index wins the tie)
    lists = [[(1, v) for v in c[2]] + [(0, 4), (2, 0), (2, BIG + 1)] for c in cases]
    st = np.full(n, 2, np.uint8)
    for val in ("middle", "min"):
        host = _host(L, U, st, lists, val)
        chosen = host[0][0::2, 1]
        assert all(int(chosen[i]) not in cases[i][2] for i in range(n))
        for reverse in (0, 1):
            _compare(_device(ctx, L, U, st, lists, val, reverse), host, st, reverse, (val, reverse))


def test_errors_leave_the_inputs_and_can_be_repeated(ctxs):
    V = 5
    ctx = ctxs(V)
    L, U, st, lists = _batch(V, 65, 9, seed=5)
    host = _host(L, U, st, lists, "middle")
    total = sum(len(r) for r in host[2])
    assert total > 0
    got = _device(ctx, L, U, st, lists, "middle", 0, capacity=total - 1)  # (_device checks the inputs and the words behind the capacity)
    assert got["counts"].tolist() == [len(host[0]), int((st == 1).sum()), int((st == 0).sum()), int((st == 2).sum()), int((st > 2).sum()), total, 1, 0]
    _compare(_device(ctx, L, U, st, lists, "middle", 0, capacity=total), host, st, 0, "repeated with room")
    # Unknown, every variable assigned (the reference panics): error 3, in a batch whose other nodes are fine
    L3, U3 = L.copy(), U.copy()
    L3[3] = U3[3]
    got = _device(ctx, L3, U3, st, lists, "middle", 0)
    assert got["counts"][6] == 3 and got["counts"][:5].tolist() == [2 * int((st == 2).sum()), int((st == 1).sum()), int((st == 0).sum()), int((st == 2).sum()), int((st > 2).sum())]
    # every value of the chosen variable excluded: error 4 (the host raises)
    L4, U4 = np.full((2, V), 1, np.int32), np.full((2, V), 1, np.int32)
    U4[:, 2] = 3
    st4 = np.full(2, 2, np.uint8)
    lists4 = [[(2, 2)], [(2, 1), (2, 3), (2, 2), (2, 2)]]
    with pytest.raises(RuntimeError, match="every value"):
        _host(L4, U4, st4, lists4, "middle")
    assert _device(ctx, L4, U4, st4, lists4, "middle", 0)["counts"][6] == 4
    _compare(_device(ctx, L4[:1], U4[:1], st4[:1], lists4[:1], "middle", 0), _host(L4[:1], U4[:1], st4[:1], lists4[:1], "middle"), st4[:1], 0, "node 0 alone")


def test_refusals():
    import torch
    dev = torch.device("cuda", 0)
    ctx = E.Context(0)
    try:
        ctx.set_model(4, np.zeros(0, dtype=M.PROP_DTYPE))
        i32 = dict(dtype=torch.int32, device=dev)
        lb, ub, st = torch.zeros((2, 4), **i32), torch.ones((2, 4), **i32), torch.full((2,), 2, dtype=torch.uint8, device=dev)
        cl, cu, coff, cex = torch.zeros((4, 4), **i32), torch.zeros((4, 4), **i32), torch.zeros(5, **i32), torch.zeros((8, 2), **i32)
        counts = torch.full((8,), -7, **i32)
        ctx.branch_device_excl(0, lb, ub, st, None, None, "middle", cl, cu, coff, cex, 8, counts)  # no nodes: PCP_OK, counts zeroed
        torch.cuda.synchronize()
        assert counts.cpu().tolist() == [0] * 8
        for bad in (dict(val=2), dict(lb=None), dict(ub=None), dict(st=None), dict(cl=None), dict(cu=None), dict(coff=None), dict(cex=None), dict(counts=None),
                    dict(off=torch.zeros(3, **i32))):  # (offsets without entries)
            a = dict(lb=lb, ub=ub, st=st, off=None, val="middle", cl=cl, cu=cu, coff=coff, cex=cex, counts=counts)
            a.update(bad)
            with pytest.raises(E.PcpError) as ei:
                ctx.branch_device_excl(2, a["lb"], a["ub"], a["st"], a["off"], None, a["val"], a["cl"], a["cu"], a["coff"], a["cex"], 8, a["counts"])
            assert ei.value.code == -1 and "pcp_branch_device_excl" in str(ei.value), bad
        ctx.set_model(4, np.zeros(0, dtype=M.PROP_DTYPE), set_words=1)
        with pytest.raises(E.PcpError) as ei:
            ctx.branch_device_excl(2, lb, ub, st, None, None, "middle", cl, cu, coff, cex, 8, counts)
        assert ei.value.code == -5 and "interval mode" in str(ei.value)
    finally:
        ctx.close()


# ---- the search -----------------------------------------------------------------------------------------------------------------------
def _queens_ctx(n):
    ctx = E.Context(0)
    ctx.set_model(n, M.nqueens_props(n))
    ctx.set_hull(1, n)
    return ctx


def _key(st):
    return st.num_nodes, st.num_solution, st.num_failed_node


@pytest.fixture(scope="module")
def queens8():
    """dfs_enumerate's trees of N-queens-8 (the tree does not depend on the batch: one host run per value selector) and dfs's solution set."""
    n = 8
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    ctx = _queens_ctx(n)
    try:
        out = {"ctx": ctx, "root": (lb0, ub0), "solutions": sorted(tuple(int(x) for x in s) for s in S.dfs(ctx, lb0, ub0, all_solutions=True, batch=64).solutions)}
        for val in ("middle", "min"):
            out[val] = {b: _key(S.dfs_enumerate(ctx, lb0, ub0, all_solutions=True, batch=b, val=val)) for b in (1, 7, 64)}
        yield out
    finally:
        ctx.close()


@pytest.mark.parametrize("val", ["middle", "min"])
def test_search_nqueens8(queens8, val):
    ctx = queens8["ctx"]
    assert len(queens8["solutions"]) == 92
    for batch in (1, 7, 64):
        for hints in (True, False):
            st = DeviceSearch(ctx, batch=batch, implicit=True, hints=hints, brancher="enumerate", val=val).run(*queens8["root"], all_solutions=True, keep_solutions=92)
            assert ctx.last_plan()["path"] == 1
            assert _key(st) == queens8[val][batch], (batch, hints)
            assert st.num_solution == 92 and sorted(tuple(int(x) for x in s) for s in st.solutions) == queens8["solutions"]
    # rows and arena so small that segments are merged, the stack compacted and rounds narrowed: the counts are unchanged
    ds = DeviceSearch(ctx, batch=7, capacity=64, excl_capacity=48, implicit=True, brancher="enumerate", val=val)
    assert _key(ds.run(*queens8["root"], all_solutions=True)) == queens8[val][7]
    assert ds.arena_events["merge"] > 0 and ds.arena_events["compact"] > 0 and (val == "min" or ds.arena_events["fewer"] > 0), ds.arena_events


def test_search_nqueens40_under_a_node_limit():
    n = 40
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    ctx = _queens_ctx(n)
    try:
        ref = S.dfs_enumerate(ctx, lb0, ub0, all_solutions=True, node_limit=2000, batch=1, val="min")
        st = DeviceSearch(ctx, batch=1, implicit=True, brancher="enumerate", val="min").run(lb0, ub0, all_solutions=True, node_limit=2000)
        assert _key(st) == _key(ref) and st.num_nodes == 2000
    finally:
        ctx.close()


def test_one_round_at_n1000():
    """64 frontier nodes of N-queens-1000 (MiddleVal: right branches carry lists): the device's own fixpoints branched on the device and by
    branch_enumerate."""
    import torch
    n = 1000
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    ctx = _queens_ctx(n)
    try:
        ds = DeviceSearch(ctx, batch=64, capacity=512, implicit=True, brancher="enumerate", val="middle")
        ds.reset(lb0, ub0)
        while ds.size < 64:
            assert not ds.advance(max_rounds=1)
        ds.compact()
        size = ds.size
        lo = size - 64
        off = ds.eoff[lo:size + 1].clone()
        lb, ub = ds.lb[lo:size].clone(), ds.ub[lo:size].clone()
        st = torch.zeros(64, dtype=torch.uint8, device=lb.device)
        ctx.propagate_device_excl(64, lb, ub, lb, ub, None, st, off, ds.ex, dirty=ds.dirty[lo:size])
        assert ctx.last_plan()["path"] == 1
        torch.cuda.synchronize()
        L, U, s, o, ex = lb.cpu().numpy(), ub.cpu().numpy(), st.cpu().numpy(), off.cpu().numpy(), ds.ex.cpu().numpy()
        lists = [[tuple(int(v) for v in p) for p in ex[o[i]:o[i + 1]]] for i in range(64)]
        assert (s == 2).sum() > 0 and sum(len(e) for e in lists) > 0
        for reverse in (0, 1):
            _compare(_device(ctx, L, U, s, lists, "middle", reverse), _host(L, U, s, lists, "middle"), s, reverse, reverse)
    finally:
        ctx.close()
