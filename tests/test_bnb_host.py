"""Branch and bound (search/branch_and_bound.rs:64-84) through the host drivers, without a GPU: `search.dfs` / `search.dfs_set` with
`objective=`, and `DeviceSearch(objective=)` over an oracle-backed stand-in of `pcp_propagate_device_bnb`.  Everything is checked
against a restatement of the reference's loop written here, over the CPU oracle, and against tests/golden/bnb_kats.json."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as orc
from oracle_ctx import OracleCtx, OracleDeviceCtx
from pcp_amd import model as M
from pcp_amd import search as S

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bnb_kats.json")))
GOLOMB = {(c["m"], c["length"]): c for c in GOLDEN["golomb_optima"]["cases"]}


# ---- the reference's loop, restated: AllSolution<OneSolution<BranchAndBound<Propagation<Brancher<FirstSmallestVar, MiddleVal, BinarySplit>>>>>
def _middle(lo, hi):
    s = int(lo) + int(hi)
    return int(np.sign(s) * (abs(s) // 2))  # Rust `/` truncates toward zero


def reference_bnb(om, lb0, ub0, var, minimize):
    """Interval mode, one node per step: the bound propagator (var < best / var > best) folded before consistency, the incumbent =
    var.lower() of every Satisfiable node, a LIFO stack with the left child on top."""
    stack = [(np.array(lb0, np.int32), np.array(ub0, np.int32))]
    r = {"nodes": 0, "failed": 0, "solutions": 0, "incumbents": [], "best": None, "row": None}
    while stack:
        L, U = (a.copy() for a in stack.pop())
        if r["best"] is not None:
            if minimize:
                U[var] = min(U[var], r["best"] - 1)
            else:
                L[var] = max(L[var], r["best"] + 1)
        r["nodes"] += 1
        if L[var] > U[var]:
            r["failed"] += 1
            continue
        lb, ub, _, st, _ = om.consistency(L[None], U[None])
        lb, ub, st = lb[0], ub[0], int(st[0])
        if st == M.FALSE:
            r["failed"] += 1
        elif st == M.TRUE:
            r["solutions"] += 1
            r["best"] = int(lb[var])
            r["incumbents"].append(r["best"])
            r["row"] = lb.copy()
        else:
            size = ub.astype(np.int64) - lb + 1
            x = min((i for i in range(len(lb)) if size[i] > 1), key=lambda i: size[i])
            v = _middle(lb[x], ub[x])
            right = (lb.copy(), ub.copy())
            right[0][x] = max(right[0][x], v + 1)
            left = (lb.copy(), ub.copy())
            left[1][x] = min(left[1][x], v)
            stack += [right, left]
    return r


def reference_bnb_set(om, lb0, ub0, var, minimize, sw, base):
    """The same over IntervalSet domains (the reference test's FDSpace): the bound clears values, FirstSmallestVar compares cardinalities."""
    vals = base + np.arange(64 * sw)

    def members(row):  # [sw] words -> sorted values
        bits = np.unpackbits(np.ascontiguousarray(row, np.uint64).view(np.uint8), bitorder="little").astype(bool)
        return vals[bits]

    def from_values(vs):
        out = np.zeros(sw, np.uint64)
        for v in vs:
            out[(v - base) // 64] |= np.uint64(1) << np.uint64((v - base) % 64)
        return out

    root = M.interval_bits(np.asarray(lb0), np.asarray(ub0), sw, base)
    stack = [root]
    r = {"nodes": 0, "failed": 0, "solutions": 0, "incumbents": [], "best": None}
    while stack:
        B = stack.pop().copy()
        if r["best"] is not None:
            keep = [v for v in members(B[var]) if (v < r["best"] if minimize else v > r["best"])]
            B[var] = from_values(keep)
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
        else:
            card = [len(members(bits[0, i])) for i in range(bits.shape[1])]
            x = min((i for i in range(len(card)) if card[i] > 1), key=lambda i: card[i])
            v = _middle(lb[0, x], ub[0, x])
            dom = members(bits[0, x])
            right, left = bits[0].copy(), bits[0].copy()
            right[x] = from_values(dom[dom > v])
            left[x] = from_values(dom[dom <= v])
            stack += [right, left]
    return r


def _golomb(m, length):
    vs, cs, var = M.golomb_ruler(m, length)
    V = len(vs)
    lb0, ub0 = vs.bounds()
    return V, cs.lower(V), lb0, ub0, var


def _kat_model():
    k = GOLDEN["reference_kats"]
    vs, cs = M.VStore(), M.CStore()
    xs = [vs.alloc((v["lb"], v["ub"])) for v in k["vars"]]
    for c in k["constraints"]:
        assert c["kind"] == "XLessY"
        cs.alloc(M.XLessY(xs[c["x"]], xs[c["y"]]))
    lb0, ub0 = vs.bounds()
    return len(vs), cs.lower(len(vs)), lb0, ub0, k["objective_var"]


class OracleSetCtx(OracleCtx):
    """OracleCtx with the set-mode entry `propagate_set` that search.dfs_set drives."""

    def __init__(self, n_vars, props, set_words, base):
        super().__init__(n_vars, props)
        self.set_words, self.base = set_words, base

    def propagate_set(self, bits, active=None, want_stats=True):
        lb, ub, b, act, st, s = self._m.consistency_set(bits, self.base, active)
        return lb, ub, b, act, st, {"steps": s["steps"], "steps3": 0}


class OracleBnbDeviceCtx(OracleDeviceCtx):
    """OracleDeviceCtx with a numpy `propagate_device_bnb`: the fold (a node it would empty keeps its row and is forced FALSE), the oracle's
    fixpoint, the reduce (best lb[var] of the TRUE nodes, the lowest index on a tie, only if it beats the incumbent)."""

    def propagate_device_bnb(self, n, lb_in, ub_in, lb_out, ub_out, active_in, active_out, status, objective, stream=0, bits_in=None, bits_out=None):
        import torch
        assert bits_in is None and bits_out is None
        self.bnb_calls = getattr(self, "bnb_calls", 0) + 1
        var, minimize = objective["var"], objective["mode"] == "min"
        best = int(objective["best"][0])
        L, U = lb_in[:n].numpy().copy(), ub_in[:n].numpy().copy()
        if minimize:
            empty = L[:, var] > best - 1
            U[~empty, var] = np.minimum(U[~empty, var], best - 1)
        else:
            empty = U[:, var] < best + 1
            L[~empty, var] = np.maximum(L[~empty, var], best + 1)
        lb_out[:n], ub_out[:n] = torch.from_numpy(L), torch.from_numpy(U)
        self.propagate_device(n, lb_out, ub_out, lb_out, ub_out, active_in, active_out, status, stream)
        st = status[:n].numpy().copy()
        st[empty] = M.FALSE
        status[:n] = torch.from_numpy(st)
        rows = np.nonzero(st == M.TRUE)[0]
        if len(rows):
            v = lb_out[:n].numpy()[rows, var]
            r = int(rows[v.argmin() if minimize else v.argmax()])
            val = int(lb_out[r, var])
            if (val < best) if minimize else (val > best):
                objective["best"][0] = val
                for k, t in (("best_lb", lb_out), ("best_ub", ub_out)):
                    if objective.get(k) is not None:
                        objective[k][:] = t[r]
                if objective.get("improved") is not None:
                    objective["improved"][0] += 1


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,length", [(5, 20), (6, 30), (7, 40)])
def test_dfs_batch1_is_the_reference_node_for_node(m, length):
    V, props, lb0, ub0, var = _golomb(m, length)
    ref = reference_bnb(orc.OracleModel(V, props), lb0, ub0, var, True)
    g = GOLOMB[(m, length)]
    assert (ref["best"], ref["nodes"], ref["failed"]) == (g["optimum"], g["nodes"], g["failed"])
    assert ref["incumbents"][-len(g["incumbents_tail"]):] == g["incumbents_tail"]
    st = S.dfs(OracleCtx(V, props), lb0, ub0, batch=1, objective=(var, "min"))
    assert (st.num_nodes, st.num_failed_node, st.num_solution) == (ref["nodes"], ref["failed"], ref["solutions"])
    assert st.incumbents == ref["incumbents"] and st.best == ref["best"]
    assert np.array_equal(st.best_solution, ref["row"])


@pytest.mark.parametrize("m,length", [(5, 20), (6, 30), (7, 40)])
def test_batched_dfs_finds_the_same_optimum(m, length):
    V, props, lb0, ub0, var = _golomb(m, length)
    st = S.dfs(OracleCtx(V, props), lb0, ub0, batch=64, objective=(var, "min"))
    assert st.best == GOLOMB[(m, length)]["optimum"]
    assert st.incumbents == sorted(st.incumbents, reverse=True) and len(set(st.incumbents)) == len(st.incumbents)
    # the row that set the incumbent is a solution: the oracle finds it Satisfiable, marks strictly increasing
    _, _, _, s, _ = orc.OracleModel(V, props).consistency(st.best_solution[None], st.best_solution[None])
    assert s[0] == M.TRUE and (np.diff(st.best_solution[:m]) > 0).all() and st.best_solution[var] == st.best


@pytest.mark.parametrize("mode", ["max", "min"])
def test_reference_kats_interval_and_set(mode):
    V, props, lb0, ub0, var = _kat_model()
    case = {c["mode"]: c for c in GOLDEN["reference_kats"]["cases"]}[mode]
    ref = reference_bnb(orc.OracleModel(V, props), lb0, ub0, var, mode == "min")
    assert ref["best"] == case["expect"] and ref["nodes"] == case["interval_nodes"]
    for batch in (1, 4):
        st = S.dfs(OracleCtx(V, props), lb0, ub0, batch=batch, objective=(var, mode))
        assert st.best == case["expect"], batch
        if batch == 1:
            assert (st.num_nodes, st.num_failed_node, st.incumbents) == (ref["nodes"], ref["failed"], ref["incumbents"])
    # FDSpace, as the reference test runs it
    ref_s = reference_bnb_set(orc.OracleModel(V, props), lb0, ub0, var, mode == "min", 1, 0)
    assert ref_s["best"] == case["expect"]
    for batch in (1, 4):
        st = S.dfs_set(OracleSetCtx(V, props, 1, 0), lb0, ub0, 0, batch=batch, objective=(var, mode))
        assert st.best == case["expect"], batch
        if batch == 1:
            assert (st.num_nodes, st.num_failed_node, st.num_solution, st.incumbents) == (ref_s["nodes"], ref_s["failed"], ref_s["solutions"], ref_s["incumbents"])


def test_objective_unset_changes_nothing():
    V, props, lb0, ub0, _ = _golomb(5, 20)
    a = S.dfs(OracleCtx(V, props), lb0, ub0, all_solutions=False, batch=1)
    b = S.dfs(OracleCtx(V, props), lb0, ub0, all_solutions=False, batch=1, objective=None)
    assert (a.num_nodes, a.num_solution, a.num_failed_node) == (b.num_nodes, b.num_solution, b.num_failed_node)
    assert b.best is None and b.best_solution is None and b.incumbents == []
    with pytest.raises(ValueError):
        S.dfs(OracleCtx(V, props), lb0, ub0, objective=(0, "smallest"))


def test_golomb_ruler_is_the_golomb_model():
    vs, cs, var = M.golomb_ruler(6, 30)
    vs2, cs2 = M.golomb(6, 30)
    assert var == 5 and np.array_equal(cs.lower(len(vs)), cs2.lower(len(vs2)))
    assert all(np.array_equal(a, b) for a, b in zip(vs.bounds(), vs2.bounds()))


def test_device_search_stand_in_batch1_is_the_reference():
    import torch
    from pcp_amd.search_device import DeviceSearch
    V, props, lb0, ub0, var = _golomb(6, 30)
    ref = reference_bnb(orc.OracleModel(V, props), lb0, ub0, var, True)
    ctx = OracleBnbDeviceCtx(V, props)
    ds = DeviceSearch(ctx, batch=1, capacity=4096, device=torch.device("cpu"), implicit=True, objective=(var, "min"))
    st = ds.run(lb0, ub0)
    assert ctx.bnb_calls == st.rounds == ref["nodes"]
    assert (st.num_nodes, st.num_failed_node, st.num_solution) == (ref["nodes"], ref["failed"], ref["solutions"])
    assert st.incumbents == ref["incumbents"] and st.best == ref["best"] == 17
    assert np.array_equal(st.best_solution, ref["row"])


@pytest.mark.parametrize("mode,expect", [("min", 0), ("max", 9)])
def test_device_search_stand_in_batched(mode, expect):
    import torch
    from pcp_amd.search_device import DeviceSearch
    V, props, lb0, ub0, var = _golomb(7, 40)
    ctx = OracleBnbDeviceCtx(V, props)
    st = DeviceSearch(ctx, batch=32, capacity=8192, device=torch.device("cpu"), implicit=True, objective=(var, "min")).run(lb0, ub0)
    assert st.best == 25 and st.best_solution[var] == 25 and len(st.incumbents) >= 1
    V, props, lb0, ub0, var = _kat_model()
    ctx = OracleBnbDeviceCtx(V, props)
    st = DeviceSearch(ctx, batch=4, capacity=256, device=torch.device("cpu"), implicit=False, objective=(var, mode)).run(lb0, ub0)
    assert st.best == expect and st.best_solution[var] == expect


def test_device_search_refuses_cells_with_an_objective():
    import torch
    from pcp_amd.search_device import DeviceSearch
    V, props, _, _, var = _golomb(5, 20)
    ctx = OracleBnbDeviceCtx(V, props)
    with pytest.raises(ValueError):
        DeviceSearch(ctx, batch=4, device=torch.device("cpu"), implicit=True, cells=True, objective=(var, "min"))
    with pytest.raises(ValueError):
        DeviceSearch(ctx, batch=4, device=torch.device("cpu"), implicit=True, objective=(var, "best"))
    with pytest.raises(ValueError):
        DeviceSearch(ctx, batch=4, device=torch.device("cpu"), implicit=True, objective=(V, "min"))
