"""Branch and bound under Enumerate over FDSpace, without a GPU: `search.dfs_enumerate_set(..., objective=)` — the host specification of the
Enumerate loop of pcp_dfs_forest_device_set_bnb — against a restatement of the reference's loop written here
(BranchAndBound<Propagation<Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate>>>, branch_and_bound.rs:64-84 + enumerate.rs:47-60),
over the CPU oracle.  tests/test_bnb_forest_gpu.py compares the device forest with the same restatement."""
import numpy as np
import pytest

from oracle import oracle as orc
from pcp_amd import model as M
from pcp_amd import search as S
from test_bnb_host import GOLOMB, OracleSetCtx, _golomb, _kat_model, reference_bnb_set


def queens6():
    """6-queens, the objective is the first queen's row."""
    n = 6
    return n, M.nqueens_props(n), np.ones(n, np.int32), np.full(n, n, np.int32), 0


# name -> (model, [(mode, the optimum known from elsewhere or None)])
MODELS = {
    "kat": (_kat_model, [("min", 0), ("max", 9)]),
    "queens6": (queens6, [("min", None), ("max", None)]),
    "golomb5": (lambda: _golomb(5, 20), [("min", GOLOMB[(5, 20)]["optimum"])]),
    "golomb6": (lambda: _golomb(6, 30), [("min", GOLOMB[(6, 30)]["optimum"])]),
}
CASES = [(name, mode, opt) for name, (_, modes) in MODELS.items() for mode, opt in modes]


def reference_bnb_set_any(om, lb0, ub0, var, minimize, sw, base, brancher="split", val="middle", best0=None):
    """The reference's loop over IntervalSet domains, one node per step, modelled on test_bnb_host.reference_bnb_set: the bound (var < best /
    var > best) folded into the node's set before consistency, a node whose set it empties counted as a node and a failure, the incumbent =
    var.lower() of every Satisfiable node, a LIFO stack with the left child on top.  brancher "split": x <= v then x > v on MiddleVal;
    "enumerate": x = v then x != v, v by the value rule of search.enumerate_value_set.  best0: an incumbent to start from."""
    root = M.interval_bits(np.asarray(lb0), np.asarray(ub0), sw, base)
    stack = [root]
    r = {"nodes": 0, "failed": 0, "solutions": 0, "incumbents": [], "best": best0, "row": None}
    while stack:
        B = stack.pop().copy()
        if r["best"] is not None:
            keep = [v for v in S.set_members(B[var], base) if (v < r["best"] if minimize else v > r["best"])]
            B[var] = 0
            for v in keep:
                B[var, (v - base) // 64] |= np.uint64(1) << np.uint64((v - base) % 64)
        r["nodes"] += 1
        if not B[var].any():
            r["failed"] += 1
            continue
        lb, ub, bits, _, st, _ = om.consistency_set(B[None], base)
        st = int(st[0])
        if st == M.FALSE:
            r["failed"] += 1
        elif st == M.TRUE:
            r["solutions"] += 1
            r["best"] = int(lb[0, var])
            r["incumbents"].append(r["best"])
            r["row"] = lb[0].copy()
        else:
            card = [len(S.set_members(bits[0, i], base)) for i in range(bits.shape[1])]
            x = min((i for i in range(len(card)) if card[i] > 1), key=lambda i: card[i])
            dom = S.set_members(bits[0, x], base)
            right, left = bits[0].copy(), bits[0].copy()
            if brancher == "enumerate":
                v = S.enumerate_value_set(bits[0, x], lb[0, x], ub[0, x], base, val)
                keep_l, keep_r = dom[dom == v], dom[dom != v]
            else:
                s = int(lb[0, x]) + int(ub[0, x])
                v = (abs(s) // 2) * (1 if s >= 0 else -1)  # Rust `/` truncates toward zero
                keep_l, keep_r = dom[dom <= v], dom[dom > v]
            for child, keep in ((left, keep_l), (right, keep_r)):
                child[x] = 0
                for u in keep:
                    child[x, (u - base) // 64] |= np.uint64(1) << np.uint64((u - base) % 64)
            stack += [right, left]
    return r


_REF = {}


def reference(name, mode, brancher="split", val="middle", best0=None):
    """The restatement's result, computed once per case and shared (never modified)."""
    key = (name, mode, brancher, val, best0)
    if key not in _REF:
        V, props, lb0, ub0, var = MODELS[name][0]()
        _REF[key] = reference_bnb_set_any(orc.OracleModel(V, props), lb0, ub0, var, mode == "min", 1, 0, brancher, val, best0)
    return _REF[key]


@pytest.mark.parametrize("name,mode,opt", CASES)
def test_the_restatement_under_binary_split_is_the_existing_one(name, mode, opt):
    V, props, lb0, ub0, var = MODELS[name][0]()
    a = reference_bnb_set(orc.OracleModel(V, props), lb0, ub0, var, mode == "min", 1, 0)
    b = reference(name, mode)
    assert all(a[k] == b[k] for k in ("nodes", "failed", "solutions", "incumbents", "best"))
    if opt is not None:
        assert b["best"] == opt


def test_counts_of_the_binary_split_cases():
    """The figures of the four cases the device test runs node for node, as measured with the restatement."""
    got = {(n, m): (reference(n, m)["nodes"], reference(n, m)["failed"], reference(n, m)["solutions"]) for n, m in
           (("queens6", "min"), ("queens6", "max"), ("golomb5", "min"), ("golomb6", "min"))}
    assert got == {("queens6", "min"): (27, 13, 1), ("queens6", "max"): (71, 32, 4), ("golomb5", "min"): (39, 18, 2), ("golomb6", "min"): (141, 68, 3)}
    assert reference("golomb5", "min")["incumbents"] == [12, 11] and reference("golomb6", "min")["incumbents"] == [20, 18, 17]


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("name,mode,opt", CASES)
def test_dfs_enumerate_set_with_an_objective_is_the_reference_node_for_node(name, mode, opt, val):
    V, props, lb0, ub0, var = MODELS[name][0]()
    ref = reference(name, mode, "enumerate", val)
    st = S.dfs_enumerate_set(OracleSetCtx(V, props, 1, 0), lb0, ub0, 0, batch=1, val=val, objective=(var, mode))
    assert (st.num_nodes, st.num_failed_node, st.num_solution) == (ref["nodes"], ref["failed"], ref["solutions"])
    assert st.incumbents == ref["incumbents"] and st.best == ref["best"]
    assert np.array_equal(st.best_solution, ref["row"])
    if opt is not None:
        assert st.best == opt
    # the optimum does not depend on the distributor
    assert st.best == reference(name, mode)["best"]


@pytest.mark.parametrize("val", ["middle", "min"])
def test_objective_unset_changes_nothing(val):
    V, props, lb0, ub0, _ = _golomb(5, 20)
    a = S.dfs_enumerate_set(OracleSetCtx(V, props, 1, 0), lb0, ub0, 0, all_solutions=True, batch=1, val=val)
    b = S.dfs_enumerate_set(OracleSetCtx(V, props, 1, 0), lb0, ub0, 0, all_solutions=True, batch=1, val=val, objective=None)
    assert (a.num_nodes, a.num_solution, a.num_failed_node) == (b.num_nodes, b.num_solution, b.num_failed_node)
    assert all(np.array_equal(x, y) for x, y in zip(a.solutions, b.solutions)) and len(a.solutions) == len(b.solutions)
    assert b.best is None and b.best_solution is None and b.incumbents == []
    # what it returns today, pinned by the plain set search: the same solutions in another order of nodes
    c = S.dfs_set(OracleSetCtx(V, props, 1, 0), lb0, ub0, 0, all_solutions=True, batch=1)
    assert c.num_solution == b.num_solution
    with pytest.raises(ValueError):
        S.dfs_enumerate_set(OracleSetCtx(V, props, 1, 0), lb0, ub0, 0, objective=(0, "smallest"))
