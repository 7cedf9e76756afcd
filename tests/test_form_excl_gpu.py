"""pcp_propagate_device_form_excl on the device (pcp_formexcl.hip, plan.path 3): nodes of a store WITH formula units (schedules) that carry
value exclusions of their own, optionally under branch and bound — and the searches built on it, search.dfs_enumerate(objective=) and
DeviceSearch(brancher="enumerate", objective=).  The oracle is the judge: every node is compared with the oracle on the store plus that node's
XNeqY(x, Constant(v)) units — the status always, the rows bit-exact when the status is not False.  The cases are form_excl_cases.py's;
test_form_excl_cpu.py holds them against the same judge without a GPU."""
import ctypes as C_

import numpy as np
import pytest

import form_excl_cases as X
from pcp_amd import model as M
from pcp_amd import search as S
import pcp_amd.engine as E

pytestmark = pytest.mark.gpu

HULL = 0xFE  # PCP_STATUS_HULL


@pytest.fixture(scope="module")
def ctx():
    c = E.Context(0)
    yield c
    c.close()


def _objective_tensors(dev, V, var, mode, best):
    import torch
    return {"var": var, "mode": mode, "best": torch.tensor([best], dtype=torch.int32, device=dev), "improved": torch.zeros(1, dtype=torch.int32, device=dev),
            "best_lb": torch.full((V,), -5, dtype=torch.int32, device=dev), "best_ub": torch.full((V,), -5, dtype=torch.int32, device=dev)}


def _run(ctx, L, U, excl, obj=None, in_place=True, lead=0, no_offsets=False):
    """One call: (lb_out, ub_out, status) as numpy, and the objective's tensors when there is one."""
    import torch
    dev = torch.device("cuda", ctx.device)
    off, flat = X.csr(excl, lead)
    lb, ub = torch.from_numpy(L.copy()).to(dev), torch.from_numpy(U.copy()).to(dev)
    lo, uo = (lb, ub) if in_place else (torch.full_like(lb, 77), torch.full_like(ub, -77))
    st = torch.full((len(L),), 255, dtype=torch.uint8, device=dev)
    t_off, t_ex = (None, None) if no_offsets else (torch.from_numpy(off).to(dev), torch.from_numpy(flat).to(dev))
    o = None if obj is None else _objective_tensors(dev, L.shape[1], *obj)
    ctx.propagate_device_form_excl(len(L), lb, ub, lo, uo, None, st, t_off, t_ex, o)
    assert ctx.last_plan()["path"] == 3
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(lb.cpu().numpy(), L) and np.array_equal(ub.cpu().numpy(), U)  # the inputs are left alone
    out = (lo.cpu().numpy(), uo.cpu().numpy(), st.cpu().numpy())
    return out if o is None else out + ({k: v.cpu().numpy() for k, v in o.items() if k not in ("var", "mode")},)


def _check(got, ref, tag=""):
    (g_lb, g_ub, g_st), (r_lb, r_ub, r_st) = got[:3], ref
    assert np.array_equal(g_st, r_st), (tag, np.nonzero(g_st != r_st)[0][:8], g_st[g_st != r_st][:8], r_st[g_st != r_st][:8])
    good = r_st != 0
    assert np.array_equal(g_lb[good], r_lb[good]) and np.array_equal(g_ub[good], r_ub[good]), tag


# ------------------------------------------------------------------------------------------------ 1. case batches
def test_per_entry_cases(ctx):
    name, L, U, excl, kinds = X.entry_cases()
    X.push(ctx, name)
    assert ctx.has_formulas and not ctx.all_neq
    ok = kinds != "badvar"
    ref = X.oracle_nodes(name, L[ok], U[ok], [e for e, o in zip(excl, ok) if o])
    for in_place in (True, False):
        got = _run(ctx, L, U, excl, in_place=in_place)
        _check(tuple(a[ok] for a in got), ref, in_place)
        # a var >= n_vars refuses ITS node and no other: PCP_STATUS_HULL, the outputs untouched
        assert (got[2][~ok] == HULL).all()
        if in_place:
            assert np.array_equal(got[0][~ok], L[~ok]) and np.array_equal(got[1][~ok], U[~ok])
        else:
            assert (got[0][~ok] == 77).all() and (got[1][~ok] == -77).all()
    with pytest.raises(E.PcpError):  # the refused node raised the sticky flag; reading it reports and clears it
        ctx.stats_read()
    ctx.stats_read()


def test_interplay_cases(ctx):
    for name, (L, U, excl, tags) in X.interplay_cases().items():
        X.push(ctx, name)
        ref = X.oracle_nodes(name, L, U, excl)
        for in_place in (True, False):
            got = _run(ctx, L, U, excl, in_place=in_place)
            _check(got, ref, (name, in_place))
            assert (got[2][tags == "a"] == 0).all() and (got[2][tags == "c"] == 2).all()


def test_chain_and_lane_stride(ctx):
    name, L, U, excl, chain = X.chain_cases()
    X.push(ctx, name)
    ctx.stats_reset()
    got = _run(ctx, L, U, excl)
    _check(got, X.oracle_nodes(name, L, U, excl), "chain")
    assert got[2][chain] == 2 and got[0][chain][1] == X.CHAIN
    s = ctx.stats_read()
    # every test of an entry is one step: the chain alone is swept 70 entries a round for at least 70 narrowing rounds and a last one
    assert s["waves"] >= X.CHAIN + 1 and s["steps"] >= (X.CHAIN + 1) * X.CHAIN
    _check(_run(ctx, L, U, excl, in_place=False), X.oracle_nodes(name, L, U, excl), "chain, out of place")


def test_more_than_64_units(ctx):
    name, L, U, excl = X.many_unit_cases()
    X.push(ctx, name)
    assert ctx.n_units > 64
    for in_place in (True, False):
        _check(_run(ctx, L, U, excl, in_place=in_place), X.oracle_nodes(name, L, U, excl), ("six", in_place))


# ------------------------------------------------------------------------------------------------ 2. launch shape
def test_more_nodes_than_wavefronts(ctx):
    """Every wavefront takes several nodes, with none / long lists / none in turn: nothing of a node's LDS state reaches the next."""
    name, BL, BU, bex = X.many_unit_cases()
    X.push(ctx, name)
    many = [e * 12 for e in bex]  # (duplicates are allowed: more than 64 entries on most nodes)
    assert max(len(e) for e in many) > 64
    nb = len(BL)
    _run(ctx, BL, BU, [[]] * nb)
    import torch
    assert ctx.last_plan()["block"] == 256
    # the grid of a large batch is what the chip holds at once (at most eight workgroups of four nodes per CU): read it from such a launch
    N0 = 8 * 4 * torch.cuda.get_device_properties(ctx.device).multi_processor_count + 5
    idx = np.arange(N0) % nb
    _run(ctx, np.ascontiguousarray(BL[idx]), np.ascontiguousarray(BU[idx]), [[]] * N0)
    plan = ctx.last_plan()
    W = plan["grid"] * plan["block"] // 64
    N = 3 * W + 5
    idx = np.arange(N) % nb
    L, U = np.ascontiguousarray(BL[idx]), np.ascontiguousarray(BU[idx])
    odd = (np.arange(N) // W) % 2 == 1
    excl = [many[b] if o else [] for b, o in zip(idx, odd)]
    got = _run(ctx, L, U, excl)
    assert ctx.last_plan() == plan and N > 2 * W  # a wavefront's nodes are W apart: it takes three of them or more
    r0, r1 = X.oracle_nodes(name, BL, BU, [[]] * nb), X.oracle_nodes(name, BL, BU, many)
    ref = tuple(np.where(odd.reshape((-1,) + (1,) * (a0.ndim - 1)), a1[idx], a0[idx]) for a0, a1 in zip(r0, r1))
    assert not np.array_equal(r0[2], r1[2]) or not np.array_equal(r0[0], r1[0]) or not np.array_equal(r0[1], r1[1])
    _check(got, ref, "node loop")


def test_csr_slices_and_null_offsets(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    name, L, U, excl, kinds = X.entry_cases()
    ok = kinds != "badvar"
    L, U, excl = np.ascontiguousarray(L[ok]), np.ascontiguousarray(U[ok]), [e for e, o in zip(excl, ok) if o]
    X.push(ctx, name)
    ref = X.oracle_nodes(name, L, U, excl)
    for in_place in (True, False):
        _check(_run(ctx, L, U, excl, lead=7, in_place=in_place), ref, ("excl_off[0] = 7", in_place))  # a slice of a larger CSR
    # no offsets: exactly propagate_device on the same rows
    a = _run(ctx, L, U, [[]] * len(L), no_offsets=True)
    lb, ub = torch.from_numpy(L.copy()).to(dev), torch.from_numpy(U.copy()).to(dev)
    st = torch.full((len(L),), 255, dtype=torch.uint8, device=dev)
    ctx.propagate_device(len(L), lb, ub, lb, ub, None, None, st)
    assert ctx.last_plan()["path"] == 3
    torch.cuda.synchronize()
    b = (lb.cpu().numpy(), ub.cpu().numpy(), st.cpu().numpy())
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _check(a, X.oracle_nodes(name, L, U, [[]] * len(L)), "no offsets")


# ------------------------------------------------------------------------------------------------ 3. branch and bound
@pytest.mark.parametrize("kind", X.BNB_KINDS)
@pytest.mark.parametrize("mode", ["min", "max"])
def test_fold_and_reduce(ctx, mode, kind):
    import torch
    dev = torch.device("cuda", ctx.device)
    name, L, U, excl, var, tie = X.bnb_batch()
    best = X.bnb_best(mode, kind, tie)
    n = X.push(ctx, name)
    lb, ub, st, emp, new_best, improved, win = X.bnb_expected(name, L, U, excl, var, mode, best)
    for in_place in (True, False):
        g_lb, g_ub, g_st, o = _run(ctx, L, U, excl, obj=(var, mode, best), in_place=in_place)
        _check((g_lb, g_ub, g_st), (lb, ub, st), (mode, best, in_place))
        # a node the fold empties: False, its output row is its input row
        assert (g_st[emp] == 0).all() and np.array_equal(g_lb[emp], L[emp]) and np.array_equal(g_ub[emp], U[emp])
        assert int(o["best"][0]) == new_best and int(o["improved"][0]) == improved
        if win is None:
            assert (o["best_lb"] == -5).all() and (o["best_ub"] == -5).all()
        else:  # of the two solutions that tie the lowest index wins
            assert np.array_equal(o["best_lb"], lb[win]) and np.array_equal(o["best_ub"], ub[win])
    # the same batch without its lists through pcp_propagate_device_bnb (fold kernel, formfix_kernel, reduce): the two agree
    none = [[] for _ in excl]
    a_lb, a_ub, a_st, a_o = _run(ctx, L, U, none, obj=(var, mode, best))
    t_lb, t_ub = torch.from_numpy(L.copy()).to(dev), torch.from_numpy(U.copy()).to(dev)
    t_st = torch.full((len(L),), 255, dtype=torch.uint8, device=dev)
    o = _objective_tensors(dev, n, var, mode, best)
    ctx.propagate_device_bnb(len(L), t_lb, t_ub, t_lb, t_ub, None, None, t_st, o)
    torch.cuda.synchronize()
    _check((a_lb, a_ub, a_st), (t_lb.cpu().numpy(), t_ub.cpu().numpy(), t_st.cpu().numpy()), "pcp_propagate_device_bnb")
    assert int(a_o["best"][0]) == int(o["best"].item()) and int(a_o["improved"][0]) == int(o["improved"].item())
    assert np.array_equal(a_o["best_lb"], o["best_lb"].cpu().numpy()) and np.array_equal(a_o["best_ub"], o["best_ub"].cpu().numpy())


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals(ctx):
    import torch
    import small_excl_cases as SX
    dev = torch.device("cuda", ctx.device)
    p = lambda t: None if t is None else C_.c_void_p(t.data_ptr())
    err = lambda: ctx._L.pcp_last_error(ctx._h).decode()

    def call(V, active_in=None, cells=False, obj=None, entry="pcp_propagate_device_form_excl"):
        lb = torch.zeros((2, V), dtype=torch.int32, device=dev)
        ub = torch.full((2, V), 5, dtype=torch.int32, device=dev)
        st = torch.zeros(2, dtype=torch.uint8, device=dev)
        off = torch.tensor([0, 1, 1], dtype=torch.int32, device=dev)
        ex = torch.tensor([[0, 3]], dtype=torch.int32, device=dev)
        bt = E.DeviceBatch(p(lb), p(ub), p(lb), p(ub), p(active_in), None, p(st), None, None, None, 1 if cells else 0, 0)
        return getattr(ctx._L, entry)(ctx._h, 2, C_.byref(bt), p(off), p(ex), None if obj is None else C_.byref(obj), C_.c_void_p(0))

    ctx.set_model(12, M.nqueens_props(12), set_words=1)  # set mode
    ctx.set_hull(1, 12)
    assert call(12) == -5 and "set mode" in err()
    n, props, lb0, ub0, gvar = SX.golomb()  # a plain store: the other two entries serve it
    ctx.set_model(n, props)
    assert not ctx.has_formulas
    assert call(n) == -5 and "formula" in err() and "pcp_propagate_device_small_excl" in err() and "pcp_propagate_device_excl" in err()
    V = X.push(ctx, "C4mk")
    var = X.store("C4mk")[2]
    assert ctx.has_formulas
    assert call(V, cells=True) == -5 and "int32 rows" in err()
    assert call(V, active_in=torch.full((2, max(ctx.words, 1)), -1, dtype=torch.int64, device=dev)) == -5 and "active_in" in err()
    assert call(V) == 0
    # a bad objective: PCP_ERR_ARG
    best = torch.tensor([X.NONE["min"]], dtype=torch.int32, device=dev)
    assert call(V, obj=E.Objective(var, 0, best.data_ptr(), None, None, None, None, 0)) == 0
    assert call(V, obj=E.Objective(V, 0, best.data_ptr(), None, None, None, None, 0)) == -1 and "objective variable" in err()   # var >= n_vars
    assert call(V, obj=E.Objective(var, 2, best.data_ptr(), None, None, None, None, 0)) == -1 and "mode" in err()               # an unknown mode
    assert call(V, obj=E.Objective(var, 0, None, None, None, None, None, 0)) == -1 and "best" in err()                          # a null best
    assert call(V, obj=E.Objective(var, 0, best.data_ptr(), None, None, None, None, 1)) == -1 and "reserved" in err()           # reserved != 0
    torch.cuda.synchronize()
    # the small-store entry keeps refusing the schedule
    assert call(V, entry="pcp_propagate_device_small_excl") == -5 and "formula" in err()


# ------------------------------------------------------------------------------------------------ 5. the search, node for node
def _counts(st):
    return (st.num_nodes, st.num_solution, st.num_failed_node, list(st.incumbents))


_SPLIT = {}


def _split_optimum(ctx, name):
    """DeviceSearch(objective=) under BinarySplit, once per model in this process (the context holds the model)."""
    from pcp_amd.search_device import DeviceSearch
    if name not in _SPLIT:
        _, _, mk, lb0, ub0, _, _ = X.store("search:" + name)
        _SPLIT[name] = DeviceSearch(ctx, batch=64, implicit=True, objective=(mk, "min")).run(lb0, ub0).best
    return _SPLIT[name]


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("name,batches", [("C4mk", (1, 3, 64)), ("D5mk", (64,))])
def test_device_search_is_dfs_enumerate_node_for_node(ctx, name, batches, val):
    """Fails without pcp_propagate_device_form_excl: both searches end in PcpError -5 "... formula ..." on their first round."""
    from pcp_amd.search_device import DeviceSearch
    key = "search:" + name
    _, _, mk, lb0, ub0, _, _ = X.store(key)
    X.push(ctx, key)
    split = _split_optimum(ctx, name)
    for batch in batches:
        limit = 300 if batch == 1 else 0  # (batch 1 is one launch per node: a few hundred of them)
        host = S.dfs_enumerate(ctx, lb0, ub0, batch=batch, val=val, objective=(mk, "min"), node_limit=limit)
        ds = DeviceSearch(ctx, batch=batch, implicit=True, brancher="enumerate", val=val, objective=(mk, "min"), capacity=4096)
        st = ds.run(lb0, ub0, node_limit=limit)
        assert ctx.last_plan()["path"] == 3 and ds.enum_form
        print(name, val, batch, _counts(st), "| host", _counts(host))
        assert _counts(st) == _counts(host), (name, val, batch)
        assert st.best == host.best
        if not limit or st.num_nodes < limit:
            assert st.best == split
            row = np.asarray(st.best_solution, np.int32)
            assert int(row[mk]) == split and int(ctx.propagate(row[None], row[None], None)[3][0]) == M.TRUE


# ------------------------------------------------------------------------------------------------ 6. all solutions, no objective
@pytest.mark.parametrize("val", ["middle", "min"])
def test_all_solutions_without_an_objective(ctx, val):
    """A4, every solution.  In interval mode a node is Satisfiable as soon as every unit is entailed, so a solution node is a BOX of schedules
    and the two distributors cut the same schedules into different boxes (379 under Enumerate / MiddleVal, 375 under BinarySplit): the sets are
    compared as sets of schedules — Enumerate's boxes hold every schedule of the model (found by trying all start times) exactly once, and
    every BinarySplit solution is one of them.  Nodes, failures and solution nodes are dfs_enumerate's."""
    from pcp_amd.search_device import DeviceSearch
    key = "search:A4"
    _, _, _, lb0, ub0, _, _ = X.store(key)
    X.push(ctx, key)
    truth = X.all_schedules("A4")
    split = DeviceSearch(ctx, batch=16, implicit=True).run(lb0, ub0, keep_solutions=4096)
    ds = DeviceSearch(ctx, batch=3, implicit=True, brancher="enumerate", val=val)
    st = ds.run(lb0, ub0, keep_solutions=4096)
    assert ds.enum_form and ctx.last_plan()["path"] == 3
    rec = []
    host = S.dfs_enumerate(ctx, lb0, ub0, all_solutions=True, batch=3, val=val, record=rec)
    assert (st.num_nodes, st.num_failed_node, st.num_solution) == (host.num_nodes, host.num_failed_node, host.num_solution)
    boxes = [(r[4], r[5]) for r in rec if r[3] == 1]
    assert len(st.solutions) == st.num_solution == len(boxes) > 0
    assert sorted(tuple(int(x) for x in s) for s in st.solutions) == sorted(tuple(int(x) for x in b[0]) for b in boxes)
    got, total = X.covered(4, boxes)
    assert got == set(truth) and total == len(truth)
    assert split.num_solution == len(split.solutions) > 0 and all(tuple(int(x) for x in s[:4]) in truth for s in split.solutions)
    assert split.num_solution == S.dfs(ctx, lb0, ub0, all_solutions=True, batch=16).num_solution
