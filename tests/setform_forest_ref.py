"""Shared by test_setform_forest_cpu.py and test_setform_forest_gpu.py: the models of the formula-store forest tests and a restatement of
the reference's search loop over FDSpace written against OracleModel.consistency_set alone — every node propagated with all units active,
as the device forest derives liveness —, under BinarySplit on MiddleVal ("split") and Enumerate on MiddleVal / MinVal, with StopNode's node
limit.  Branch and bound is test_bnb_forest_cpu.reference_bnb_set_any, which takes any OracleModel.  Results are computed once per
process and never modified."""
import functools

import numpy as np

from pcp_amd import model as M
from pcp_amd import search as S

import setform_cases as SC

DUR4, DUR5 = (2, 3, 2, 1), (3, 2, 4, 2, 3)


@functools.lru_cache(maxsize=None)
def schedule(durations=DUR4, horizon=8, makespan=False):
    """setform_cases.disjunctive_schedule, optionally with a makespan variable m in [0, horizon] (the last variable) and s_i + d_i <= m for
    every task.  Returns (vs, cs, index of m or None)."""
    vs, cs, s, _ = SC.disjunctive_schedule(durations, horizon)
    m = None
    if makespan:
        mv = vs.alloc((0, horizon))
        m = len(vs) - 1
        for si, d in zip(s, durations):
            cs.alloc(M.x_leq_y(M.Addition(si, d), mv))
    return vs, cs, m


def schedule_is_valid(sol, durations=DUR4, makespan=None):
    """test_setform_gpu.schedule_is_valid for any durations: no two tasks overlap, b == (s_0 < s_2), and every task ends by `makespan`."""
    n = len(durations)
    s = [int(v) for v in sol[:n]]
    pairs = all(s[i] + durations[i] <= s[j] or s[j] + durations[j] <= s[i] for i in range(n) for j in range(i + 1, n))
    ends = makespan is None or all(s[i] + durations[i] <= makespan for i in range(n))
    return pairs and ends and (int(sol[n]) == 1) == (s[0] < s[2])


def _with(row, x, keep, base):
    out = row.copy()
    out[x] = 0
    for u in keep:
        out[x, (int(u) - base) // 64] |= np.uint64(1) << np.uint64((int(u) - base) % 64)
    return out


def reference_search(om, root_bits, base, brancher="split", val="middle", node_limit=0):
    """All solutions below root_bits ([V, sw] uint64), one node per step, a LIFO stack with the left child on top.  A node: consistency
    with every unit active; False = a failure, True = a solution (its lower bounds), Unknown = a branch on the variable of minimal
    cardinality > 1, first index — "split": x <= v then x > v, v = (lower + upper) / 2 truncated toward zero; "enumerate": x = v then
    x != v, v by search.enumerate_value_set.  node_limit: the node that reaches it is explored and counted but is neither a solution nor a
    failure, and the search ends (stop_node.rs:55-62)."""
    stack = [np.array(root_bits, dtype=np.uint64)]
    r = {"nodes": 0, "solutions": 0, "failed": 0, "rows": []}
    while stack:
        B = stack.pop()
        r["nodes"] += 1
        last = bool(node_limit) and r["nodes"] >= node_limit
        lb, ub, bits, _, st, _ = om.consistency_set(B[None], base)
        st = int(st[0])
        if st == M.FALSE:
            r["failed"] += 0 if last else 1
        elif st == M.TRUE:
            if not last:
                r["solutions"] += 1
                r["rows"].append(lb[0].copy())
        else:
            card = [len(S.set_members(bits[0, i], base)) for i in range(bits.shape[1])]
            x = min((i for i in range(len(card)) if card[i] > 1), key=lambda i: card[i])
            dom = S.set_members(bits[0, x], base)
            if brancher == "enumerate":
                v = S.enumerate_value_set(bits[0, x], lb[0, x], ub[0, x], base, val)
                keep_l, keep_r = dom[dom == v], dom[dom != v]
            else:
                s = int(lb[0, x]) + int(ub[0, x])
                v = (abs(s) // 2) * (1 if s >= 0 else -1)
                keep_l, keep_r = dom[dom <= v], dom[dom > v]
            stack += [_with(bits[0], x, keep_r, base), _with(bits[0], x, keep_l, base)]
        if last:
            break
    return r


@functools.lru_cache(maxsize=None)
def schedule_counts(durations, horizon, makespan, brancher="split", val="middle", node_limit=0, sw=1, base=0):
    """(nodes, solutions, failed) of reference_search on a schedule model from its hull."""
    vs, cs, _ = schedule(durations, horizon, makespan)
    r = reference_search(SC.oracle_model(vs, cs), SC.hull_sets(vs, sw, base), base, brancher, val, node_limit)
    return r["nodes"], r["solutions"], r["failed"]


@functools.lru_cache(maxsize=None)
def schedule_bnb(durations, horizon, brancher="split", val="middle"):
    """Minimising the makespan with test_bnb_forest_cpu.reference_bnb_set_any: its result dict."""
    from test_bnb_forest_cpu import reference_bnb_set_any
    vs, cs, m = schedule(durations, horizon, True)
    lb0, ub0 = vs.bounds()
    return reference_bnb_set_any(SC.oracle_model(vs, cs), lb0, ub0, m, True, 1, 0, brancher, val)


BRANCHERS = [("split", "middle"), ("enumerate", "middle"), ("enumerate", "min")]
