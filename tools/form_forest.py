"""The search forest over an Interval store with formula units against the two other ways such a store is searched on the device today, all
three in one process on one context: a Cumulative schedule of five tasks (durations 3,2,2,1,2, resources 2,1,2,1,1, capacity 3, starts
0..7: 46 variables; with --makespan-model durations 3,2,4,1,2, starts 0..8 and a makespan variable 0..14 for branch and bound).
  1. the complete tree:
       forest         search_forest.forest_search(formulas=True) — one tree per wavefront, the node in LDS (pcp_dfs_forest_device_form) — with
                      each number of --trees;
       dfs_device     Context.dfs_device — pcp_dfs_device: three launches per node, one wavefront busy — on the first --dfs-nodes nodes;
       device_search  DeviceSearch at --batch (pcp_propagate_device + pcp_branch_device: a row per open node in HBM).
  2. the makespan minimised: search_forest.forest_bnb with the same numbers of trees, and DeviceSearch(objective=...).
One warm-up run of each, then the faster of two.  Prints one JSON line per run: nodes, launches (rounds for DeviceSearch), seconds, nodes/s.
The complete-tree runs must agree on nodes / solutions / failed; the minimisations visit different trees and must agree on the optimum.

    python tools/form_forest.py [--trees 1,64,1024,8192] [--steps 512] [--batch 1024] [--dfs-nodes 20000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def schedule(durations, resources, horizon, makespan):
    from pcp_amd import model as M
    vs, cs = M.VStore(), M.CStore()
    s = [vs.alloc((0, horizon)) for _ in durations]
    mk = vs.alloc((0, makespan)) if makespan else None
    cap = vs.alloc((3, 3))
    M.Cumulative(s, [M.Constant(d) for d in durations], [M.Constant(r) for r in resources], cap).join(vs, cs)
    if mk is not None:
        for si, d in zip(s, durations):
            cs.alloc(M.x_leq_y(M.Addition(si, d), mk))
    return vs, cs, (mk.idx if mk is not None else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", default="1,64,1024,8192")
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dfs-nodes", type=int, default=20000)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import pcp_amd.engine as E
    from pcp_amd import model as M
    from pcp_amd.search_device import DeviceSearch
    from pcp_amd.search_forest import forest_bnb, forest_search

    trees = [int(x) for x in args.trees.split(",")]
    gpu = torch.cuda.get_device_name(0)
    ctx = E.Context(0)

    def timed(fn, warm=None):
        (warm or fn)()  # warm-up: allocations, the first launch of every kernel
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

    def emit(workload, what, engine, nodes, launches, t, **more):
        print(json.dumps({"tool": "form_forest", "workload": workload, "what": what, "engine": engine, "gpu": gpu, "nodes": nodes, "launches": launches,
                          "seconds": round(t, 5), "nodes_per_s": round(nodes / t, 1), **more}), flush=True)

    # ---- 1. the complete tree --------------------------------------------------------------------------------------------------------------
    work = "cumulative(3,2,2,1,2 / 2,1,2,1,1 / 3, starts 0..7)"
    vs, cs, _ = schedule((3, 2, 2, 1, 2), (2, 1, 2, 1, 1), 7, 0)
    lb0, ub0 = vs.bounds()
    M.push_model(ctx, cs, len(vs))
    seen = set()
    for T in trees:
        r, t = timed(lambda: forest_search(ctx, lb0, ub0, n_trees=T, steps_per_launch=args.steps, formulas=True))
        assert r["error"] == 0, r
        seen.add((r["nodes"], r["solutions"], r["failed"]))
        emit(work, "complete tree", "forest", r["nodes"], r["launches"], t, n_trees=r["trees"], steps_per_launch=args.steps, solutions=r["solutions"],
             failed=r["failed"], seeded_nodes=r["seeded_nodes"], plan=ctx.last_plan())
    ds = DeviceSearch(ctx, batch=args.batch, capacity=64 * args.batch + 4096, implicit=True)
    d, t = timed(lambda: ds.run(lb0, ub0, all_solutions=True, keep_solutions=0))
    seen.add((d.num_nodes, d.num_solution, d.num_failed_node))
    emit(work, "complete tree", "device_search", d.num_nodes, d.rounds, t, batch=args.batch, solutions=d.num_solution, failed=d.num_failed_node)
    assert len(seen) == 1, seen
    one = lambda limit: ctx.dfs_device(lb0, ub0, 1 << 30, capacity=256, stop_on_solution=False, node_limit=limit, chunk=1024)
    r, t = timed(lambda: one(args.dfs_nodes), warm=lambda: one(256))
    emit(work, f"the first {args.dfs_nodes} nodes", "dfs_device", r["nodes"], r["steps_enqueued"], t, solutions=r["solutions"], failed=r["failed"])

    # ---- 2. the makespan minimised -----------------------------------------------------------------------------------------------------------
    work = "cumulative(3,2,4,1,2 / 2,1,2,1,1 / 3, starts 0..8, makespan 0..14)"
    vs, cs, m = schedule((3, 2, 4, 1, 2), (2, 1, 2, 1, 1), 8, 14)
    lb0, ub0 = vs.bounds()
    M.push_model(ctx, cs, len(vs))
    optimum = set()
    for T in trees:
        r, t = timed(lambda: forest_bnb(ctx, lb0, ub0, (m, "min"), n_trees=T, steps_per_launch=args.steps))
        assert r["error"] == 0 and r["open"] == 0, r
        optimum.add(r["best"])
        emit(work, "minimise the makespan", "forest", r["nodes"], r["launches"], t, n_trees=r["trees"], steps_per_launch=args.steps, best=r["best"],
             solutions=r["solutions"], failed=r["failed"], seeded_nodes=r["seeded_nodes"])
    ds = DeviceSearch(ctx, batch=args.batch, capacity=64 * args.batch + 4096, implicit=True, objective=(m, "min"))
    d, t = timed(lambda: ds.run(lb0, ub0))
    optimum.add(d.best)
    emit(work, "minimise the makespan", "device_search", d.num_nodes, d.rounds, t, batch=args.batch, best=d.best, solutions=d.num_solution, failed=d.num_failed_node)
    assert optimum == {7}, optimum
    ctx.close()


if __name__ == "__main__":
    main()
