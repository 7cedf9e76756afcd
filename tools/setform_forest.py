"""The search forest over a formula store against the batched device search, both on one set-mode context: a disjunctive schedule of six
tasks on one machine (pairwise Or(s_i + d_i <= s_j, s_j + d_j <= s_i), one equivalence(Boolean(b), s_0 < s_2)), horizon large enough for a
few hundred thousand nodes.
  1. all solutions: search_forest.forest_search_set(formulas=True) — one tree per wavefront, the node in LDS, an undo trail
     (pcp_dfs_forest_device_setform) — with each number of --trees, and DeviceSearch at --batch (pcp_propagate_device + pcp_branch_device_set:
     a full row per open node in HBM);
  2. the makespan minimised: forest_bnb_set(formulas=True) with the same numbers of trees, and DeviceSearch(objective=...).
One warm-up run of each, then the faster of two.  Prints one JSON line per run: nodes, launches (rounds for DeviceSearch), seconds, nodes/s.
The all-solutions runs must agree on nodes / solutions / failed; the minimisations visit different trees and must agree on the optimum.

    python tools/setform_forest.py [--durations 3,2,4,2,3,1] [--horizon 20] [--trees 64,512,4096] [--steps 2048] [--batch 1024] [--brancher split] [--val middle]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def schedule(durations, horizon, makespan):
    from pcp_amd import model as M
    vs, cs = M.VStore(), M.CStore()
    s = [vs.alloc((0, horizon - d)) for d in durations]
    b = vs.alloc((0, 1))
    for i in range(len(s)):
        for j in range(i + 1, len(s)):
            cs.alloc(M.Or((M.x_leq_y(M.Addition(s[i], durations[i]), s[j]), M.x_leq_y(M.Addition(s[j], durations[j]), s[i]))))
    cs.alloc(M.equivalence(M.Boolean(b), M.XLessY(s[0], s[2])))
    m = None
    if makespan:
        mv = vs.alloc((0, horizon))
        m = len(vs) - 1
        for si, d in zip(s, durations):
            cs.alloc(M.x_leq_y(M.Addition(si, d), mv))
    return vs, cs, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--durations", default="3,2,4,2,3,1")
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--trees", default="64,512,4096")
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--ramp", type=int, default=16)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--brancher", default="split")
    ap.add_argument("--val", default="middle")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import pcp_amd.engine as E
    from pcp_amd import model as M
    from pcp_amd.search_device import DeviceSearch
    from pcp_amd.search_forest import forest_bnb_set, forest_search_set

    durations = tuple(int(x) for x in args.durations.split(","))
    trees = [int(x) for x in args.trees.split(",")]
    gpu = torch.cuda.get_device_name(0)
    ctx = E.Context(0)

    def timed(fn):
        fn()  # warm-up: allocations, the first launch of every kernel
        best = None
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            if best is None or t < best[1]:
                best = (r, t)
        return best

    def emit(what, engine, nodes, launches, t, **more):
        print(json.dumps({"tool": "setform_forest", "workload": f"disjunctive_schedule({list(durations)}, {args.horizon})", "what": what, "engine": engine, "gpu": gpu,
                          "brancher": args.brancher, "val": args.val, "nodes": nodes, "launches": launches, "seconds": round(t, 5), "nodes_per_s": round(nodes / t, 1),
                          **more}), flush=True)

    # ---- 1. all solutions ------------------------------------------------------------------------------------------------------------------
    vs, cs, _ = schedule(durations, args.horizon, False)
    lb0, ub0 = vs.bounds()
    M.push_model(ctx, cs, len(vs), 1)
    ctx.set_hull(0, 63)
    seen = set()
    for T in trees:
        r, t = timed(lambda: forest_search_set(ctx, lb0, ub0, 0, n_trees=T, steps_per_launch=args.steps, brancher=args.brancher, val=args.val, formulas=True))
        assert r["error"] == 0 and r["finished_trees"] == r["trees"], r
        seen.add((r["nodes"], r["solutions"], r["failed"]))
        emit("all solutions", "forest", r["nodes"], r["launches"], t, n_trees=r["trees"], steps_per_launch=args.steps, solutions=r["solutions"], failed=r["failed"],
             seeded_nodes=r["seeded_nodes"], splits=r["splits"], plan=ctx.last_plan())
    ds = DeviceSearch(ctx, batch=args.batch, capacity=64 * args.batch + 4096, implicit=True, brancher=args.brancher, val=args.val)
    d, t = timed(lambda: ds.run(lb0, ub0, all_solutions=True, keep_solutions=0, base=0))
    seen.add((d.num_nodes, d.num_solution, d.num_failed_node))
    emit("all solutions", "device_search", d.num_nodes, d.rounds, t, batch=args.batch, solutions=d.num_solution, failed=d.num_failed_node)
    assert len(seen) == 1, seen

    # ---- 2. the makespan minimised -----------------------------------------------------------------------------------------------------------
    vs, cs, m = schedule(durations, args.horizon, True)
    lb0, ub0 = vs.bounds()
    M.push_model(ctx, cs, len(vs), 1)
    ctx.set_hull(0, 63)
    optimum = set()
    for T in trees:
        r, t = timed(lambda: forest_bnb_set(ctx, lb0, ub0, 0, (m, "min"), n_trees=T, ramp_steps=args.ramp, steps_per_launch=args.steps, brancher=args.brancher,
                                            val=args.val, formulas=True))
        assert r["error"] == 0 and r["finished_trees"] == T, r
        optimum.add(r["best"])
        emit("minimise the makespan", "forest", r["nodes"], r["launches"], t, n_trees=T, ramp_steps=args.ramp, steps_per_launch=args.steps, best=r["best"],
             solutions=r["solutions"], failed=r["failed"], splits=r["splits"])
    ds = DeviceSearch(ctx, batch=args.batch, capacity=64 * args.batch + 4096, implicit=True, brancher=args.brancher, val=args.val, objective=(m, "min"))
    d, t = timed(lambda: ds.run(lb0, ub0, base=0))
    optimum.add(d.best)
    emit("minimise the makespan", "device_search", d.num_nodes, d.rounds, t, batch=args.batch, best=d.best, solutions=d.num_solution, failed=d.num_failed_node)
    assert len(optimum) == 1 and sum(durations) in optimum, optimum
    ctx.close()


if __name__ == "__main__":
    main()
