"""pcp_propagate_device_form_excl, the parts that need no GPU: the ABI lists, the cases of form_excl_cases.py against the judge (the oracle on
the store plus that node's XNeqY(x, Constant v) units), and `search.dfs_enumerate(objective=)` / `DeviceSearch(brancher="enumerate",
objective=)` over an oracle-backed stand-in context that says `has_formulas` against a restatement of the reference's loop written here
(BranchAndBound<Propagation<Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate>>>, branch_and_bound.rs:64-84 + enumerate.rs:47-60)."""
import os

import numpy as np
import pytest

import form_excl_cases as X
import small_excl_cases as SX
from pcp_amd import search as S
import pcp_amd.engine as E
from pcp_amd.search_device import DeviceSearch
from test_enum_search_cpu import EnumOracleCtx
from test_small_excl_cpu import SmallExclOracleCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_lists_the_entry():
    assert "pcp_propagate_device_form_excl" in E.ABI_SYMBOLS  # (tests/test_abi.py then checks the header and the export)
    rust = open(os.path.join(ROOT, "integration", "pcp-hip-sys", "src", "lib.rs")).read()
    assert "pcp_propagate_device_form_excl" in rust
    assert hasattr(E.Context, "propagate_device_form_excl") and isinstance(E.Context.has_formulas, property)
    import __graft_entry__ as g
    assert g.HIP_OBJECTS["formexcl.o"][0].endswith("pcp_formexcl.hip")


# ------------------------------------------------------------------------------------------------ the cases against the judge
def sweep_then_units(name, L, U, ex):
    """(status, lb, ub) of one node as the kernel's rounds compute it: the exclusion sweep (small_excl_cases.sweep) and the fixpoint of the
    store WITHOUT the node's units (the oracle's) in turn, until nothing moves."""
    om = X.model_with(name)
    lb, ub = L.copy(), U.copy()
    while True:
        l1, u1, failed, opened, _ = SX.sweep(lb, ub, ex)
        if failed or (l1 > u1).any():
            return 0, lb, ub
        r = om.consistency(l1[None], u1[None], None)
        if int(r[3][0]) == 0:
            return 0, lb, ub
        l2, u2 = r[0][0], r[1][0]
        if np.array_equal(l2, lb) and np.array_equal(u2, ub):
            return (2 if (opened or int(r[3][0]) == 2) else 1), lb, ub
        lb, ub = l2.copy(), u2.copy()


def _check_interleaved(name, L, U, excl, skip=()):
    """sweeping the lists next to the units reaches the fixpoint of the store with the XNeqY units allocated behind it."""
    for i in range(len(L)):
        if i in skip:
            continue
        want, got = X.judge(name, L[i], U[i], excl[i]), sweep_then_units(name, L[i], U[i], excl[i])
        assert got[0] == want[0], (name, i, excl[i], got[0], want[0])
        if want[0] != 0:
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (name, i, excl[i])


def test_entry_cases_have_every_kind():
    name, L, U, excl, kinds = X.entry_cases()  # (what each kind shows is asserted on the oracle where the cases are built)
    assert tuple(kinds) == X.ENTRY_KINDS and len(excl) == len(L) == len(kinds)
    assert max(a for e in excl for a, _ in e) == L.shape[1]  # the malformed entry names the first index that is no variable
    _check_interleaved(name, L, U, excl, skip={int(np.nonzero(kinds == "badvar")[0][0])})


def test_interplay_cases():
    cases = X.interplay_cases()
    for name, (L, U, excl, tags) in cases.items():
        assert (tags == "a").sum() >= 2 and (tags == "b").sum() >= 2
        _check_interleaved(name, L, U, excl)
        ref = X.oracle_nodes(name, L, U, excl)
        assert (ref[2][tags == "a"] == 0).all() and (ref[2][tags == "b"] != 0).all() and (ref[2][tags == "c"] == 2).all()


def test_chain_and_many_units():
    name, L, U, excl, chain = X.chain_cases()
    # only one value falls per sweep when the order never meets the bound: 70 narrowing rounds
    l, u, rounds = L[chain].copy(), U[chain].copy(), 0
    while True:
        l2, u2, failed, _, steps = SX.sweep(l, u, sorted(excl[chain], reverse=True))
        assert not failed and steps == X.CHAIN
        if np.array_equal(l2, l):
            break
        l, rounds = l2, rounds + 1
    assert rounds == X.CHAIN
    _check_interleaved(name, L, U, excl)
    name, L, U, excl = X.many_unit_cases()
    _check_interleaved(name, L, U, excl)


def test_bnb_batch_and_the_fold():
    name, L, U, excl, var, tie = X.bnb_batch()
    assert 8 <= len(L) <= 10
    plain = X.oracle_nodes(name, L, U, excl)
    assert plain[2][3] == plain[2][4] == 1 and plain[0][3][var] == plain[0][4][var] == tie  # two solutions that tie
    assert (L[:, var] >= 0).all() and (U[:, var] <= 12).all()
    for mode, best in X.bnb_bests(tie):
        lb, ub, st, emp, new_best, improved, win = X.bnb_expected(name, L, U, excl, var, mode, best)
        if best in X.NONE.values():  # "no solution yet" moves nothing; of the two that tie the lowest index wins
            assert not emp.any() and np.array_equal(st, plain[2]) and improved == 1 and win == 3 and new_best == tie
        elif (mode, best) in (("min", 14), ("max", -1)):  # a bound no node reaches: nothing moves, the first solution improves on it
            assert not emp.any() and np.array_equal(st, plain[2]) and win == 3
        elif (mode, best) in (("min", -1), ("max", 14)):  # a bound beyond every node: all are emptied, rows unchanged
            assert emp.all() and (st == 0).all() and np.array_equal(lb, L) and np.array_equal(ub, U) and win is None and new_best == best
        elif mode == "min":  # equal to the makespan of the two: both emptied
            assert emp[3] and emp[4] and not emp.all() and win is None
        else:  # Maximize from the makespan of the two: their makespan variable is still open above it
            assert not emp[3] and st[3] == 1 and lb[3][var] == tie + 1 and win is not None and new_best > tie


# ------------------------------------------------------------------------------------------------ the search
class FormExclOracleCtx(EnumOracleCtx):
    """EnumOracleCtx over a store with formula units, plus `has_formulas` and `propagate_device_form_excl`: the fold, the judge per node, the
    reduce — form_excl_cases.bnb_expected.  The two older entries refuse, as the engine does."""

    def __init__(self, name):
        n = len(X.store(name)[0])
        super().__init__(n, np.zeros(0, dtype=SX.M.PROP_DTYPE))
        self._name, self._m = name, X.model_with(name)
        self.n_units, self.words = self._m.n_units, self._m.words
        self.has_formulas = True
        self.all_neq = False
        self.form_calls = 0

    def propagate_device_excl(self, *a, **k):
        raise AssertionError("a store with formula units: pcp_propagate_device_form_excl is the entry")

    propagate_device_small_excl = propagate_device_excl

    def propagate_device_form_excl(self, n, lb_in, ub_in, lb_out, ub_out, active_out, status, excl_off, excl, objective=None, stream=0):
        import torch
        assert active_out is None
        self.form_calls += 1
        L, U = lb_in[:n].numpy().copy(), ub_in[:n].numpy().copy()
        off, ex = excl_off[:n + 1].numpy(), excl.numpy()
        lists = [[(int(a), int(b)) for a, b in ex[off[i]:off[i + 1]]] for i in range(n)]
        if objective is None:
            lb, ub, st = X.oracle_nodes(self._name, L, U, lists)
        else:
            lb, ub, st, _, best, improved, win = X.bnb_expected(self._name, L, U, lists, objective["var"], objective["mode"], int(objective["best"][0]))
            if win is not None:
                objective["best"][0] = best
                objective["improved"][0] += improved
                objective["best_lb"][:] = torch.from_numpy(lb[win])
                objective["best_ub"][:] = torch.from_numpy(ub[win])
        lb_out[:n], ub_out[:n], status[:n] = torch.from_numpy(lb), torch.from_numpy(ub), torch.from_numpy(st)
        self._stats["nodes"] += n


def reference_bnb_enum(name, lb0, ub0, var, mode, val):
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
        st, lb, ub = X.judge(name, L, U, ex)
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


def _objective(name):
    """The makespan, minimised; A4 has none: its last task as late as possible."""
    mk = X.store("search:" + name)[2]
    return (mk, "min") if mk is not None else (3, "max")


SEARCH_NAMES = ("A4", "C4mk", "D5mk")
_REF = {}


def reference(name, val):
    if (name, val) not in _REF:
        _, _, _, lb0, ub0, _, _ = X.store("search:" + name)
        var, mode = _objective(name)
        _REF[(name, val)] = reference_bnb_enum("search:" + name, lb0, ub0, var, mode, val)
    return _REF[(name, val)]


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("name", SEARCH_NAMES)
def test_searches_are_the_reference_node_for_node(name, val):
    """dfs_enumerate(objective=) and DeviceSearch(brancher="enumerate", objective=) over the stand-in: the restatement at batch 1, each other at
    batches 3 and 64, the same optimum at every batch; every launch is propagate_device_form_excl."""
    import torch
    key = "search:" + name
    _, _, _, lb0, ub0, _, _ = X.store(key)
    var, mode = _objective(name)
    ref = reference(name, val)
    print(name, val, "reference:", ref["nodes"], "nodes", ref["solutions"], "solutions", ref["failed"], "failed", ref["incumbents"])
    assert 0 < ref["nodes"] <= X.TREE_CEILING and ref["solutions"] >= 1
    for batch in (1, 3, 64):
        ctx = FormExclOracleCtx(key)
        host = S.dfs_enumerate(ctx, lb0, ub0, batch=batch, val=val, objective=(var, mode))
        assert ctx.form_calls > 0 and host.num_nodes <= X.TREE_CEILING
        ctx = FormExclOracleCtx(key)
        # (capacity: a row buffer that runs short makes DeviceSearch take fewer nodes a round, which under branch and bound is another order
        # than the host's; D5mk holds up to some 650 open nodes at batch 64)
        ds = DeviceSearch(ctx, batch=batch, device=torch.device("cpu"), implicit=True, brancher="enumerate", val=val, objective=(var, mode), capacity=4096)
        assert ds.enum_form and ds.enum_small and ds.dirty is None
        st = ds.run(lb0, ub0)
        assert ctx.form_calls == st.rounds
        assert (st.num_nodes, st.num_solution, st.num_failed_node) == (host.num_nodes, host.num_solution, host.num_failed_node), batch
        assert st.incumbents == host.incumbents and st.best == host.best == ref["best"] and int(st.best_solution[var]) == ref["best"]
        if batch == 1:
            assert (host.num_nodes, host.num_failed_node, host.num_solution) == (ref["nodes"], ref["failed"], ref["solutions"])
            assert host.incumbents == ref["incumbents"] and np.array_equal(host.best_solution, ref["row"])
            assert np.array_equal(st.best_solution, ref["row"])
    if X.store(key)[2] is not None:  # the optimum is a schedule, and no shorter one exists: BinarySplit on the same stand-in agrees
        assert S.dfs(FormExclOracleCtx(key), lb0, ub0, objective=(var, mode), batch=1).best == ref["best"]


def test_all_solutions_without_an_objective_take_the_new_entry_too():
    """A4 without an objective: the Satisfiable nodes are boxes (form_excl_cases.covered) that hold every schedule of the model once, under
    either value selector; BinarySplit cuts the same schedules into other boxes."""
    import torch
    key = "search:A4"
    _, _, _, lb0, ub0, _, _ = X.store(key)
    truth = X.all_schedules("A4")
    assert len(truth) > 100
    for val in ("middle", "min"):
        ctx, rec = FormExclOracleCtx(key), []
        a = S.dfs_enumerate(ctx, lb0, ub0, all_solutions=True, batch=4, val=val, record=rec)
        assert ctx.form_calls > 0 and a.best is None and 0 < a.num_nodes <= X.TREE_CEILING
        boxes = [(r[4], r[5]) for r in rec if r[3] == 1]
        got, total = X.covered(4, boxes)
        assert len(boxes) == a.num_solution and got == set(truth) and total == len(truth)
        ctx = FormExclOracleCtx(key)
        ds = DeviceSearch(ctx, batch=4, device=torch.device("cpu"), implicit=True, brancher="enumerate", val=val)
        st = ds.run(lb0, ub0, keep_solutions=4096)
        assert ds.enum_form and ds.dirty is None and ctx.form_calls == st.rounds
        assert (st.num_nodes, st.num_solution, st.num_failed_node) == (a.num_nodes, a.num_solution, a.num_failed_node)
        assert sorted(tuple(int(x) for x in s) for s in st.solutions) == sorted(tuple(int(x) for x in b[0]) for b in boxes)
    split = DeviceSearch(FormExclOracleCtx(key), batch=4, device=torch.device("cpu"), implicit=True).run(lb0, ub0, keep_solutions=4096)
    assert split.num_solution == len(split.solutions) > 0 and all(tuple(int(x) for x in s[:4]) in truth for s in split.solutions)


def test_a_context_without_has_formulas_takes_the_old_entries():
    """The dispatch changes for no other context: one that does not have the attribute (or has it False) goes where it went."""
    import torch
    from pcp_amd import model as M
    V, props, lb0, ub0, var = SX.golomb(5, 11)
    for flag in (None, False):
        ctx = SmallExclOracleCtx(V, props)
        if flag is not None:
            ctx.has_formulas = flag
        ctx.propagate_device_form_excl = None  # (calling it would raise)
        assert not hasattr(SmallExclOracleCtx, "has_formulas")
        host = S.dfs_enumerate(ctx, lb0, ub0, batch=3, objective=(var, "min"))
        assert ctx.small_calls > 0 and host.best == 11
        ctx = SmallExclOracleCtx(V, props)
        if flag is not None:
            ctx.has_formulas = flag
        ds = DeviceSearch(ctx, batch=3, device=torch.device("cpu"), implicit=True, brancher="enumerate", objective=(var, "min"))
        assert ds.enum_small and not ds.enum_form
        st = ds.run(lb0, ub0)
        assert ctx.small_calls == st.rounds and st.best == 11 and st.incumbents == host.incumbents
    q = EnumOracleCtx(6, M.nqueens_props(6))  # an all-XNeqY store that says nothing: pcp_propagate_device_excl and its hints
    ds = DeviceSearch(q, batch=4, device=torch.device("cpu"), implicit=True, brancher="enumerate")
    assert not ds.enum_small and not ds.enum_form and ds.dirty is not None
