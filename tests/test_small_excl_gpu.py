"""pcp_propagate_device_small_excl on the device (pcp_smallexcl.hip, plan.path 4): nodes of a small store of any plain model with value
exclusions of their own, optionally under branch and bound — and the searches built on it, search.dfs_enumerate(objective=) and
DeviceSearch(brancher="enumerate", objective=).  The oracle is the judge: every node is compared with OracleModel(n, props + that node's
XNeqY(x, Constant(v)) units).consistency on the same row — the status always, the rows bit-exact when the status is not False.  The cases are
small_excl_cases.py's; test_small_excl_cpu.py holds them against the same judge without a GPU."""
import ctypes as C_

import numpy as np
import pytest

import small_excl_cases as X
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


def _run(ctx, L, U, excl, obj=None, in_place=True, lead=0, no_offsets=False):
    """One call: (lb_out, ub_out, status) as numpy, and the objective's tensors when there is one."""
    import torch
    dev = torch.device("cuda", ctx.device)
    off, flat = X.csr(excl, lead)
    lb, ub = torch.from_numpy(L.copy()).to(dev), torch.from_numpy(U.copy()).to(dev)
    lo, uo = (lb, ub) if in_place else (torch.full_like(lb, 77), torch.full_like(ub, -77))
    st = torch.full((len(L),), 255, dtype=torch.uint8, device=dev)
    t_off, t_ex = (None, None) if no_offsets else (torch.from_numpy(off).to(dev), torch.from_numpy(flat).to(dev))
    o = None
    if obj is not None:
        var, mode, best = obj
        o = {"var": var, "mode": mode, "best": torch.tensor([best], dtype=torch.int32, device=dev), "improved": torch.zeros(1, dtype=torch.int32, device=dev),
             "best_lb": torch.full((L.shape[1],), -5, dtype=torch.int32, device=dev), "best_ub": torch.full((L.shape[1],), -5, dtype=torch.int32, device=dev)}
    ctx.propagate_device_small_excl(len(L), lb, ub, lo, uo, None, st, t_off, t_ex, o)
    assert ctx.last_plan()["path"] == 4
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


# ------------------------------------------------------------------------------------------------ 1. per-entry cases
@pytest.mark.parametrize("which", ["queens", "golomb"])
def test_per_entry_cases(ctx, which):
    n, props, L, U, excl, kind = X.entry_cases(which)
    ctx.set_model(n, props)
    assert not ctx.all_neq
    ok = kind != "badvar"
    ref = X.oracle_nodes(n, props, L[ok], U[ok], [e for e, o in zip(excl, ok) if o])
    for in_place in (True, False):
        got = _run(ctx, L, U, excl, in_place=in_place)
        _check(tuple(a[ok] for a in got), ref, (which, in_place))
        # a var >= n_vars refuses ITS node and no other: PCP_STATUS_HULL, the outputs untouched
        assert (got[2][~ok] == HULL).all()
        if in_place:
            assert np.array_equal(got[0][~ok], L[~ok]) and np.array_equal(got[1][~ok], U[~ok])
        else:
            assert (got[0][~ok] == 77).all() and (got[1][~ok] == -77).all()
    with pytest.raises(E.PcpError):  # the refused nodes raised the sticky flag; reading it reports and clears it
        ctx.stats_read()
    ctx.stats_read()


# ------------------------------------------------------------------------------------------------ 2. lane-stride and round seams
def test_lane_stride_and_round_seams(ctx):
    n, props, L, U, excl, chain = X.seam_cases()
    ctx.set_model(n, props)
    ctx.stats_reset()
    got = _run(ctx, L, U, excl)
    _check(got, X.oracle_nodes(n, props, L, U, excl), "seams")
    assert got[2][chain] != 0 and got[0][chain][5] == L[chain][5] + 70
    s = ctx.stats_read()
    # every test of an entry is one step: the chain alone is swept 70 entries a round for at least 70 narrowing rounds and a last one
    assert s["waves"] >= 71 and s["steps"] >= 71 * 70 + sum(X.SEAM_COUNTS)
    n, props, L, U, excl, _ = X.alldiff_cases()
    ctx.set_model(n, props)
    for alldiff in (1, 0):  # the value mask and the pairs: the same fixpoint
        ctx.set_option("small_alldiff", alldiff)
        try:
            got = _run(ctx, L, U, excl)
        finally:
            ctx.set_option("small_alldiff", 1)
        _check(got, X.oracle_nodes(n, props, L, U, excl), ("alldiff", alldiff))


# ------------------------------------------------------------------------------------------------ 3. launch shape
def test_more_nodes_than_wavefronts(ctx):
    """Every wavefront takes several nodes, with 0 / many / 0 entries in turn."""
    n, props, BL, BU, bex, _ = X.alldiff_cases()
    ctx.set_model(n, props)
    many = [e * 8 for e in bex]  # (duplicates are allowed: more than 64 entries on most nodes)
    assert max(len(e) for e in many) > 64
    nb, N = len(BL), 3 * 8192 + 5
    idx = np.arange(N) % nb
    L, U = np.ascontiguousarray(BL[idx]), np.ascontiguousarray(BU[idx])
    _run(ctx, L, U, [[]] * N)
    plan = ctx.last_plan()
    W = plan["grid"] * plan["block"] // 64
    assert plan["block"] == 256 and N > 2 * W  # a wavefront's nodes are W apart: it takes three of them or more
    odd = (np.arange(N) // W) % 2 == 1
    excl = [many[b] if o else [] for b, o in zip(idx, odd)]
    got = _run(ctx, L, U, excl)
    assert ctx.last_plan() == plan
    r0, r1 = X.oracle_nodes(n, props, BL, BU, [[]] * nb), X.oracle_nodes(n, props, BL, BU, many)
    ref = tuple(np.where(odd.reshape((-1,) + (1,) * (a0.ndim - 1)), a1[idx], a0[idx]) for a0, a1 in zip(r0, r1))
    assert not np.array_equal(r0[2], r1[2]) or not np.array_equal(r0[0], r1[0]) or not np.array_equal(r0[1], r1[1])
    _check(got, ref, "node loop")


def test_csr_slices_null_offsets_and_the_old_entry(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    n, props, L, U, excl, kind = X.entry_cases("golomb")
    ok = kind != "badvar"
    L, U, excl = L[ok], U[ok], [e for e, o in zip(excl, ok) if o]
    ctx.set_model(n, props)
    ref = X.oracle_nodes(n, props, L, U, excl)
    for in_place in (True, False):
        _check(_run(ctx, L, U, excl, lead=7, in_place=in_place), ref, ("excl_off[0] = 7", in_place))  # a slice of a larger CSR
    # no offsets: exactly propagate_device on the same rows
    a = _run(ctx, L, U, [[]] * len(L), no_offsets=True)
    lb, ub = torch.from_numpy(L.copy()).to(dev), torch.from_numpy(U.copy()).to(dev)
    st = torch.full((len(L),), 255, dtype=torch.uint8, device=dev)
    ctx.propagate_device(len(L), lb, ub, lb, ub, None, None, st)
    torch.cuda.synchronize()
    _check(a, (lb.cpu().numpy(), ub.cpu().numpy(), st.cpu().numpy()), "propagate_device")
    _check(a, X.oracle_nodes(n, props, L, U, [[]] * len(L)), "no offsets")
    # an all-XNeqY model within the limits is accepted too: the results of pcp_propagate_device_excl on the same batch
    n, _, L, U, excl, kind = X.entry_cases("queens")
    props = M.nqueens_props(n)
    ctx.set_model(n, props)
    assert ctx.all_neq
    new = _run(ctx, L, U, excl)
    off, flat = X.csr(excl)
    lb, ub = torch.from_numpy(L.copy()).to(dev), torch.from_numpy(U.copy()).to(dev)
    st = torch.full((len(L),), 255, dtype=torch.uint8, device=dev)
    ctx.propagate_device_excl(len(L), lb, ub, lb, ub, None, st, torch.from_numpy(off).to(dev), torch.from_numpy(flat).to(dev))
    assert ctx.last_plan()["path"] == 1
    torch.cuda.synchronize()
    old = (lb.cpu().numpy(), ub.cpu().numpy(), st.cpu().numpy())
    assert (old[2][kind == "badvar"] == HULL).all()
    _check(new, old, "the old entry")
    ok = kind != "badvar"
    _check(tuple(a[ok] for a in new), X.oracle_nodes(n, props, L[ok], U[ok], [e for e, o in zip(excl, ok) if o]), "all-XNeqY")
    with pytest.raises(E.PcpError):
        ctx.stats_read()
    ctx.stats_read()


# ------------------------------------------------------------------------------------------------ 4. branch and bound
BNB_CASES = [("min", X.NONE["min"]), ("min", 12), ("min", 11), ("min", 8), ("max", X.NONE["max"]), ("max", 8), ("max", 10), ("max", 11)]


@pytest.mark.parametrize("mode,best", BNB_CASES)
def test_fold_and_reduce(ctx, mode, best):
    import torch
    dev = torch.device("cuda", ctx.device)
    n, props, L, U, excl, var = X.bnb_batch()
    ctx.set_model(n, props)
    lb, ub, st, emp, new_best, improved, win = X.bnb_expected(n, props, L, U, excl, var, mode, best)
    if best in X.NONE.values():  # no incumbent: the fold is a no-op, the two solutions tie and the lowest index wins
        assert not emp.any() and improved == 1 and win == 6 and st[6] == st[7] == 1 and new_best == 11
        plain = X.oracle_nodes(n, props, L, U, excl)
        assert np.array_equal(plain[2], st)
    if (mode, best) in (("min", 11), ("min", 8), ("max", 11)):
        assert emp.any()  # the fold empties nodes
    if (mode, best) in (("min", 11), ("min", 8), ("max", 8), ("max", 10)):
        assert any(not emp[i] and ((U[i, var] > best - 1) if mode == "min" else (L[i, var] < best + 1)) for i in range(len(L)))  # ... and narrows others
    for in_place in (True, False):
        g_lb, g_ub, g_st, o = _run(ctx, L, U, excl, obj=(var, mode, best), in_place=in_place)
        _check((g_lb, g_ub, g_st), (lb, ub, st), (mode, best, in_place))
        # a node the fold empties: False, its output row is its input row
        assert (g_st[emp] == 0).all() and np.array_equal(g_lb[emp], L[emp]) and np.array_equal(g_ub[emp], U[emp])
        assert int(o["best"][0]) == new_best and int(o["improved"][0]) == improved
        if win is None:
            assert (o["best_lb"] == -5).all() and (o["best_ub"] == -5).all()
        else:
            assert np.array_equal(o["best_lb"], lb[win]) and np.array_equal(o["best_ub"], ub[win])
    # the same batch without its exclusions through pcp_propagate_device_bnb (fold kernel, fixpoint, reduce): where that path applies — it
    # takes no lists — the two agree
    none = [[] for _ in excl]
    a_lb, a_ub, a_st, a_o = _run(ctx, L, U, none, obj=(var, mode, best))
    t_lb, t_ub = torch.from_numpy(L.copy()).to(dev), torch.from_numpy(U.copy()).to(dev)
    t_st = torch.full((len(L),), 255, dtype=torch.uint8, device=dev)
    o = {"var": var, "mode": mode, "best": torch.tensor([best], dtype=torch.int32, device=dev), "improved": torch.zeros(1, dtype=torch.int32, device=dev),
         "best_lb": torch.full((n,), -5, dtype=torch.int32, device=dev), "best_ub": torch.full((n,), -5, dtype=torch.int32, device=dev)}
    ctx.propagate_device_bnb(len(L), t_lb, t_ub, t_lb, t_ub, None, None, t_st, o)
    torch.cuda.synchronize()
    _check((a_lb, a_ub, a_st), (t_lb.cpu().numpy(), t_ub.cpu().numpy(), t_st.cpu().numpy()), "pcp_propagate_device_bnb")
    assert int(a_o["best"][0]) == int(o["best"].item()) and int(a_o["improved"][0]) == int(o["improved"].item())
    assert np.array_equal(a_o["best_lb"], o["best_lb"].cpu().numpy()) and np.array_equal(a_o["best_ub"], o["best_ub"].cpu().numpy())


def test_exclusions_agree_with_node_units(ctx):
    """The lists as pcp_propagate_device_units rows on smallfix_kernel: the same statuses and rows."""
    import torch
    dev = torch.device("cuda", ctx.device)
    for n, props, L, U, excl in (X.seam_cases()[:5], X.alldiff_cases()[:5], X.bnb_batch()[:5]):
        ctx.set_model(n, props)
        new = _run(ctx, L, U, excl)
        off, _ = X.csr(excl)
        flat = np.concatenate([X.units(e) for e in excl if len(e)])
        lb, ub = torch.from_numpy(L.copy()).to(dev), torch.from_numpy(U.copy()).to(dev)
        st = torch.full((len(L),), 255, dtype=torch.uint8, device=dev)
        ctx.propagate_device_units(len(L), lb, ub, lb, ub, None, None, st, torch.from_numpy(off).to(dev), torch.from_numpy(flat.view(np.uint8).copy()).to(dev))
        assert ctx.last_plan()["path"] == 4
        torch.cuda.synchronize()
        _check(new, (lb.cpu().numpy(), ub.cpu().numpy(), st.cpu().numpy()), "node units")


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(ctx):
    import torch
    import form_forest_cases as FC
    import small_forest_cases as SF
    dev = torch.device("cuda", ctx.device)
    p = lambda t: None if t is None else C_.c_void_p(t.data_ptr())

    def call(V, active_in=None, cells=False, obj=None):
        lb = torch.zeros((2, V), dtype=torch.int32, device=dev)
        ub = torch.full((2, V), 5, dtype=torch.int32, device=dev)
        st = torch.zeros(2, dtype=torch.uint8, device=dev)
        off = torch.tensor([0, 1, 1], dtype=torch.int32, device=dev)
        ex = torch.tensor([[0, 3]], dtype=torch.int32, device=dev)
        bt = E.DeviceBatch(p(lb), p(ub), p(lb), p(ub), p(active_in), None, p(st), None, None, None, 1 if cells else 0, 0)
        return ctx._L.pcp_propagate_device_small_excl(ctx._h, 2, C_.byref(bt), p(off), p(ex), None if obj is None else C_.byref(obj), C_.c_void_p(0))

    ctx.set_model(12, M.nqueens_props(12), set_words=1)  # set mode
    ctx.set_hull(1, 12)
    assert call(12) == -5 and "set mode" in ctx._L.pcp_last_error(ctx._h).decode()
    n, props, lb0, ub0, var = X.golomb()
    vs, cs, _ = FC.schedule("A4")  # a store with formula units
    M.push_model(ctx, cs, len(vs))
    assert call(len(vs)) == -5 and "formula" in ctx._L.pcp_last_error(ctx._h).decode()
    vs, cs = SF.slots129()  # one slot beyond the limit
    M.push_model(ctx, cs, len(vs))
    assert call(len(vs)) == -5 and "128" in ctx._L.pcp_last_error(ctx._h).decode()
    ctx.set_model(n, props)
    assert call(n, cells=True) == -5
    assert call(n, active_in=torch.full((2, max(ctx.words, 1)), -1, dtype=torch.int64, device=dev)) == -5
    assert call(n) == 0
    # a bad objective: PCP_ERR_ARG
    best = torch.tensor([X.NONE["min"]], dtype=torch.int32, device=dev)
    assert call(n, obj=E.Objective(var, 0, best.data_ptr(), None, None, None, None, 0)) == 0
    assert call(n, obj=E.Objective(n, 0, best.data_ptr(), None, None, None, None, 0)) == -1     # var >= n_vars
    assert call(n, obj=E.Objective(var, 2, best.data_ptr(), None, None, None, None, 0)) == -1   # an unknown mode
    assert call(n, obj=E.Objective(var, 0, None, None, None, None, None, 0)) == -1              # a null best
    assert call(n, obj=E.Objective(var, 0, best.data_ptr(), None, None, None, None, 1)) == -1   # reserved != 0
    torch.cuda.synchronize()
    # the old entry keeps refusing this model
    with pytest.raises(E.PcpError) as e:
        lb = torch.zeros((1, n), dtype=torch.int32, device=dev)
        ctx.propagate_device_excl(1, lb, lb, lb, lb, None, torch.zeros(1, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int32, device=dev),
                                  torch.zeros((1, 2), dtype=torch.int32, device=dev))
    assert e.value.code == -5


# ------------------------------------------------------------------------------------------------ 6. the search, node for node
def _counts(st):
    return (st.num_nodes, st.num_solution, st.num_failed_node, list(st.incumbents))


_SPLIT = {}


def _split_optimum(ctx, m, length):
    """DeviceSearch(objective=) under BinarySplit, once per model in this process."""
    from pcp_amd.search_device import DeviceSearch
    if (m, length) not in _SPLIT:
        n, props, lb0, ub0, var = X.golomb(m, length)
        _SPLIT[(m, length)] = DeviceSearch(ctx, batch=64, implicit=True, objective=(var, "min")).run(lb0, ub0).best
    return _SPLIT[(m, length)]


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("m,length,batches", [(5, 11, (1, 3, 64)), (6, 17, (1, 3, 64)), (7, 25, (64,))])
def test_device_search_is_dfs_enumerate_node_for_node(ctx, m, length, batches, val):
    from pcp_amd.search_device import DeviceSearch
    n, props, lb0, ub0, var = X.golomb(m, length)
    ctx.set_model(n, props)
    split = _split_optimum(ctx, m, length)
    assert split == length == {5: 11, 6: 17, 7: 25}[m]
    for batch in batches:
        host = S.dfs_enumerate(ctx, lb0, ub0, batch=batch, val=val, objective=(var, "min"))
        ds = DeviceSearch(ctx, batch=batch, implicit=True, brancher="enumerate", val=val, objective=(var, "min"))
        st = ds.run(lb0, ub0)
        assert ctx.last_plan()["path"] == 4 and ds.enum_small
        print("golomb", m, val, batch, _counts(st), "| host", _counts(host))
        assert _counts(st) == _counts(host), (m, val, batch)
        assert st.best == host.best == split
        row = np.asarray(st.best_solution, np.int32)
        assert int(row[var]) == split and int(ctx.propagate(row[None], row[None], None)[3][0]) == M.TRUE


# ------------------------------------------------------------------------------------------------ 7. all solutions, no objective
@pytest.mark.parametrize("val", ["middle", "min"])
def test_all_solutions_without_an_objective(ctx, val):
    from pcp_amd.search_device import DeviceSearch
    n, props, lb0, ub0, var = X.golomb(5, 11)
    ctx.set_model(n, props)
    split = DeviceSearch(ctx, batch=16, implicit=True).run(lb0, ub0, keep_solutions=64)
    ds = DeviceSearch(ctx, batch=3, implicit=True, brancher="enumerate", val=val, capacity=20, excl_capacity=30)
    st = ds.run(lb0, ub0, keep_solutions=64)
    host = S.dfs_enumerate(ctx, lb0, ub0, all_solutions=True, batch=3, val=val)
    assert ds.enum_small and ctx.last_plan()["path"] == 4
    assert st.num_solution == split.num_solution == host.num_solution > 0
    assert (st.num_nodes, st.num_failed_node) == (host.num_nodes, host.num_failed_node)
    assert sorted(tuple(int(x) for x in s) for s in st.solutions) == sorted(tuple(int(x) for x in s) for s in split.solutions)
    ev = ds.arena_events
    assert ev["merge"] > 0 and ev["compact"] > 0, ev
