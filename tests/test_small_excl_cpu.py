"""pcp_propagate_device_small_excl, the parts that need no GPU: the ABI lists, the cases of small_excl_cases.py and its scalar restatement of
the kernel's exclusion sweep and fold against the oracle (every node judged by OracleModel(n, props + that node's XNeqY(x, Constant v)
units).consistency), and `search.dfs_enumerate(objective=)` / `DeviceSearch(brancher="enumerate", objective=)` on an oracle-backed stand-in
context against a restatement of the reference's loop written here
(BranchAndBound<Propagation<Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate>>>, branch_and_bound.rs:64-84 + enumerate.rs:47-60)."""
import os

import numpy as np
import pytest

import small_excl_cases as X
from pcp_amd import search as S
import pcp_amd.engine as E
from pcp_amd.search_device import DeviceSearch
from test_bnb_host import _kat_model
from test_enum_search_cpu import EnumOracleCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_lists_the_entry():
    assert "pcp_propagate_device_small_excl" in E.ABI_SYMBOLS  # (tests/test_abi.py then checks the header and the export)
    rust = open(os.path.join(ROOT, "integration", "pcp-hip-sys", "src", "lib.rs")).read()
    assert "pcp_propagate_device_small_excl" in rust and "pub struct pcp_objective" in rust
    assert hasattr(E.Context, "propagate_device_small_excl") and hasattr(E.Context, "all_neq")


# ------------------------------------------------------------------------------------------------ the cases and the restatement
def _check_restated(n, props, L, U, excl, skip=()):
    for i in range(len(L)):
        if i in skip:
            continue
        want, got = X.judge(n, props, L[i], U[i], excl[i]), X.restated(n, props, L[i], U[i], excl[i])
        assert got[0] == want[0], (i, excl[i], got[0], want[0])
        if want[0] != 0:
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (i, excl[i])


@pytest.mark.parametrize("which", ["queens", "golomb"])
def test_entry_cases_have_every_kind_and_the_restatement_is_the_oracle(which):
    n, props, L, U, excl, kind = X.entry_cases(which)
    for k in X.ENTRY_KINDS:
        assert (kind == k).any(), k
    base = X.oracle_nodes(n, props, L, U, [[] for _ in excl])
    ok = kind != "badvar"
    ref = X.oracle_nodes(n, props, L[ok], U[ok], [e for e, o in zip(excl, ok) if o])
    assert (ref[2][kind[ok] == "assigned_same"] == 0).all()  # x assigned to the excluded value: the node fails
    for k in ("at_lb", "at_ub", "dups"):  # a value at a bound goes: the oracle's answer differs from its answer without the entries
        sel = np.nonzero(kind[ok] == k)[0]
        assert any(ref[2][i] != base[2][ok][i] or not np.array_equal(ref[0][i], base[0][ok][i]) or not np.array_equal(ref[1][i], base[1][ok][i]) for i in sel), k
    for k in ("interior",):  # a value inside removes nothing and keeps the node Unknown
        for i in np.nonzero(kind[ok] == k)[0]:
            assert ref[2][i] == 2 and np.array_equal(ref[0][i], base[0][ok][i]) and np.array_equal(ref[1][i], base[1][ok][i])
    for k in ("outside", "assigned_other"):  # entailed from the start: the node is what it is without them
        for i in np.nonzero(kind[ok] == k)[0]:
            assert ref[2][i] == base[2][ok][i]
    _check_restated(n, props, L, U, excl, skip=set(np.nonzero(~ok)[0]))


def test_seam_cases_and_the_chain():
    n, props, L, U, excl, chain = X.seam_cases()
    assert tuple(len(e) for e in excl[:len(X.SEAM_COUNTS)]) == X.SEAM_COUNTS and len(excl[chain]) == 70
    st, lb, ub = X.judge(n, props, L[chain], U[chain], excl[chain])
    assert st != 0 and lb[5] == L[chain][5] + 70  # the chain ends at lb + 70
    # ... and only one value falls per sweep: the restatement's sequential pass in an order that never meets the bound needs them all
    l, u, rounds = L[chain].copy(), U[chain].copy(), 0
    while True:
        l2, u2, failed, _, steps = X.sweep(l, u, sorted(excl[chain], reverse=True))
        assert not failed and steps == 70
        if np.array_equal(l2, l):
            break
        l, rounds = l2, rounds + 1
    assert rounds == 70
    _check_restated(n, props, L, U, excl)


def test_alldiff_cases():
    n, props, L, U, excl, m = X.alldiff_cases()
    assert all(a >= m for e in excl for a, _ in e) and any(len(e) >= 4 for e in excl)
    assert any((L[i][m:] == U[i][m:]).any() for i in range(len(L)))  # assigned differences: the value mask has bits
    ref = X.oracle_nodes(n, props, L, U, excl)
    base = X.oracle_nodes(n, props, L, U, [[] for _ in excl])
    assert not (np.array_equal(ref[2], base[2]) and np.array_equal(ref[0], base[0]) and np.array_equal(ref[1], base[1]))
    _check_restated(n, props, L, U, excl)


def test_fold_restated_against_the_bound_propagator():
    """The fold is XLessY(var, Constant(best)) / x_greater_y(var, Constant(best)) run once: the oracle on a store of that one propagator."""
    n, props, L, U, excl, var = X.bnb_batch()
    for mode, bests in (("min", (X.NONE["min"], 12, 11, 8, 1, 0)), ("max", (X.NONE["max"], -1, 5, 9, 11, 12))):
        for best in bests:
            p = np.zeros(1, dtype=props.dtype)
            p["kind"] = 2  # XLessY
            p["var"][0] = [var, 0xFFFFFFFF, 0xFFFFFFFE] if mode == "min" else [0xFFFFFFFF, var, 0xFFFFFFFE]
            p["off"][0][1 if mode == "min" else 0] = best
            om = X.plain_model(n, p)
            for i in range(len(L)):
                fl, fu, emptied = X.fold(L[i], U[i], var, mode, best)
                r = om.consistency(L[i][None], U[i][None], None)
                assert emptied == (int(r[3][0]) == 0), (mode, best, i)
                if emptied:
                    assert np.array_equal(fl, L[i]) and np.array_equal(fu, U[i])
                else:
                    assert np.array_equal(fl, r[0][0]) and np.array_equal(fu, r[1][0])
    exp = X.bnb_expected(n, props, L, U, excl, var, "min", X.NONE["min"])
    assert exp[4] == 11 and exp[5] == 1 and exp[6] == 6 and not exp[3].any()  # two solutions tie: the first wins
    exp = X.bnb_expected(n, props, L, U, excl, var, "min", 11)
    assert exp[5] == 0 and exp[6] is None and exp[3][6] and exp[3][7] and (exp[2][6:8] == 0).all()  # the solutions are emptied


# ------------------------------------------------------------------------------------------------ the search
class SmallExclOracleCtx(EnumOracleCtx):
    """EnumOracleCtx plus `propagate_device_small_excl`: the fold, the judge per node, the reduce — small_excl_cases.bnb_expected."""

    def __init__(self, n_vars, props):
        super().__init__(n_vars, props)
        self.all_neq = False
        self.small_calls = 0

    def propagate_device_excl(self, *a, **k):
        raise AssertionError("a store that is not all-XNeqY, or an objective: pcp_propagate_device_small_excl is the entry")

    def propagate_device_small_excl(self, n, lb_in, ub_in, lb_out, ub_out, active_out, status, excl_off, excl, objective=None, stream=0):
        import torch
        assert active_out is None
        self.small_calls += 1
        L, U = lb_in[:n].numpy().copy(), ub_in[:n].numpy().copy()
        off, ex = excl_off[:n + 1].numpy(), excl.numpy()
        lists = [[(int(a), int(b)) for a, b in ex[off[i]:off[i + 1]]] for i in range(n)]
        if objective is None:
            lb, ub, st = X.oracle_nodes(self.n_vars, self._props, L, U, lists)
        else:
            mode = objective["mode"]
            lb, ub, st, _, best, improved, win = X.bnb_expected(self.n_vars, self._props, L, U, lists, objective["var"], mode, int(objective["best"][0]))
            if win is not None:
                objective["best"][0] = best
                objective["improved"][0] += improved
                objective["best_lb"][:] = torch.from_numpy(lb[win])
                objective["best_ub"][:] = torch.from_numpy(ub[win])
        lb_out[:n], ub_out[:n], status[:n] = torch.from_numpy(lb), torch.from_numpy(ub), torch.from_numpy(st)
        self._stats["nodes"] += n


def reference_bnb_enum(n, props, lb0, ub0, var, mode, val):
    """The reference's loop, one node per step: the bound folded before consistency, a node it empties counted as a node and a failure, the
    incumbent = var.lower() of every Satisfiable node, Enumerate's children (x = v on top, then x != v: folded at a bound, carried inside)."""
    stack = [(np.array(lb0, np.int32), np.array(ub0, np.int32), np.zeros((0, 2), np.int32))]
    r = {"nodes": 0, "failed": 0, "solutions": 0, "incumbents": [], "best": None, "row": None}
    while stack:
        L, U, ex = stack.pop()
        r["nodes"] += 1
        if r["best"] is not None:
            L, U, emptied = X.fold(L, U, var, mode, r["best"])
            if emptied:
                r["failed"] += 1
                continue
        st, lb, ub = X.judge(n, props, L, U, ex)
        if st == 0:
            r["failed"] += 1
        elif st == 1:
            r["solutions"] += 1
            r["best"] = int(lb[var])
            r["incumbents"].append(r["best"])
            r["row"] = lb.copy()
        else:
            cl, cu, coff, cex, _ = S.branch_enumerate(lb, ub, [0, len(ex)], ex, val=val)
            stack.append((cl[1], cu[1], cex[coff[1]:coff[2]].copy()))
            stack.append((cl[0], cu[0], cex[coff[0]:coff[1]].copy()))
    return r


def _golomb5():
    return X.golomb(5, 11)


SEARCH_CASES = [("kat", "min", 0), ("kat", "max", 9), ("golomb5", "min", 11)]
_MODELS = {"kat": _kat_model, "golomb5": _golomb5}
_REF = {}


def reference(name, mode, val):
    key = (name, mode, val)
    if key not in _REF:
        V, props, lb0, ub0, var = _MODELS[name]()
        _REF[key] = reference_bnb_enum(V, props, lb0, ub0, var, mode, val)
    return _REF[key]


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("name,mode,opt", SEARCH_CASES)
def test_dfs_enumerate_with_an_objective_is_the_reference_node_for_node(name, mode, opt, val):
    V, props, lb0, ub0, var = _MODELS[name]()
    ref = reference(name, mode, val)
    assert ref["best"] == opt
    ctx = SmallExclOracleCtx(V, props)
    st = S.dfs_enumerate(ctx, lb0, ub0, batch=1, val=val, objective=(var, mode))
    assert ctx.small_calls > 0
    assert (st.num_nodes, st.num_failed_node, st.num_solution) == (ref["nodes"], ref["failed"], ref["solutions"])
    assert st.incumbents == ref["incumbents"] and st.best == opt
    assert np.array_equal(st.best_solution, ref["row"])
    # the optimum does not depend on the distributor, nor on the batch
    assert S.dfs(ctx, lb0, ub0, objective=(var, mode), batch=1).best == opt
    assert S.dfs_enumerate(ctx, lb0, ub0, batch=5, val=val, objective=(var, mode)).best == opt


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("name,mode,opt", SEARCH_CASES)
def test_device_search_under_enumerate_with_an_objective(name, mode, opt, val):
    """The open-node stack, the arena and the round buffer (the incumbent behind the brancher's eight counts) on CPU tensors."""
    import torch
    V, props, lb0, ub0, var = _MODELS[name]()
    for batch in (1, 3, 64):
        host = S.dfs_enumerate(SmallExclOracleCtx(V, props), lb0, ub0, batch=batch, val=val, objective=(var, mode))
        ctx = SmallExclOracleCtx(V, props)
        ds = DeviceSearch(ctx, batch=batch, device=torch.device("cpu"), implicit=True, brancher="enumerate", val=val, objective=(var, mode))
        assert ds.enum_small and ds.dirty is None
        st = ds.run(lb0, ub0)
        assert (st.num_nodes, st.num_solution, st.num_failed_node) == (host.num_nodes, host.num_solution, host.num_failed_node), batch
        assert st.incumbents == host.incumbents and st.best == opt and int(st.best_solution[var]) == opt
        if batch == 1:
            ref = reference(name, mode, val)
            assert (st.num_nodes, st.num_failed_node, st.num_solution) == (ref["nodes"], ref["failed"], ref["solutions"])


def test_without_an_objective_a_mixed_store_takes_the_new_entry_and_an_all_xneqy_store_the_old_one():
    import torch
    from pcp_amd import model as M
    V, props, lb0, ub0, var = _golomb5()
    ctx = SmallExclOracleCtx(V, props)
    a = S.dfs_enumerate(ctx, lb0, ub0, all_solutions=True, batch=4, val="middle")
    assert ctx.small_calls > 0 and a.best is None and a.incumbents == []
    split = S.dfs(ctx, lb0, ub0, all_solutions=True, batch=4)
    assert a.num_solution == split.num_solution > 0
    ds = DeviceSearch(SmallExclOracleCtx(V, props), batch=4, device=torch.device("cpu"), implicit=True, brancher="enumerate", capacity=64, excl_capacity=40)
    st = ds.run(lb0, ub0)
    assert ds.enum_small and (st.num_nodes, st.num_solution, st.num_failed_node) == (a.num_nodes, a.num_solution, a.num_failed_node)
    # an all-XNeqY store (a context that says so, or says nothing) keeps pcp_propagate_device_excl and its hints
    n = 6
    q = EnumOracleCtx(n, M.nqueens_props(n))
    ds = DeviceSearch(q, batch=4, device=torch.device("cpu"), implicit=True, brancher="enumerate")
    assert not ds.enum_small and ds.dirty is not None
    q.all_neq = True
    assert not DeviceSearch(q, batch=4, device=torch.device("cpu"), implicit=True, brancher="enumerate").enum_small
    with pytest.raises(ValueError, match="objective"):
        S.dfs_enumerate(ctx, lb0, ub0, objective=(var, "smallest"))
