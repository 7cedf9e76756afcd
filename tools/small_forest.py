#!/usr/bin/env python
"""The search forest over small Interval stores (pcp_dfs_forest_device_small_bnb) on the shortest Golomb ruler, against the two other ways
the device searches this store, all in one process on one context: model.golomb_ruler(m, LENGTH[m]) for m = 8, 9, 10 (the lengths and
optima of tools/bnb_golomb.py), the last mark minimised.
    forest         search_forest.forest_bnb(small=True) — one tree per wavefront, the node in LDS, the records in the workgroup's LDS copy —
                   at each number of --trees;
    device_search  DeviceSearch(objective=) at each --batch (pcp_propagate_device_bnb + pcp_branch_device: a row per open node in HBM);
    dfs_device     Context.dfs_device — pcp_dfs_device: three launches per node, one tree, no objective — on the first --dfs-nodes nodes.
One warm-up of each entry on m = 8, then every case once.  Prints one JSON line per case: optimum, nodes, seconds, nodes/s.  The
minimisations visit different trees (the incumbent arrives at different moments) and must agree on the optimum.

    python tools/small_forest.py [--m 8,9,10] [--trees 256,4096,13824] [--batch 1024,4096] [--steps 512] [--dfs-nodes 5000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bnb_golomb import LENGTH, OPTIMUM  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", default="8,9,10")
    ap.add_argument("--trees", default="256,4096,13824")
    ap.add_argument("--batch", default="1024,4096")
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--dfs-nodes", type=int, default=5000)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import pcp_amd.engine as E
    from pcp_amd import model as M
    from pcp_amd.search_device import DeviceSearch
    from pcp_amd.search_forest import forest_bnb

    ints = lambda s: [int(x) for x in s.split(",") if x]
    gpu = torch.cuda.get_device_name(0)
    ctx = E.Context(0)
    ctx.set_option("time_kernels", 0)  # no event pair around every launch

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def emit(m, how, size, optimum, nodes, dt, **more):
        print(json.dumps({"gpu": gpu, "m": m, "length": LENGTH[m], "how": how, "size": size, "optimum": optimum, "expected": OPTIMUM[m],
                          "ok": optimum is None or optimum == OPTIMUM[m], "nodes": nodes, "seconds": round(dt, 4), "nodes_per_s": round(nodes / dt, 1), **more}), flush=True)

    warm = True
    for m in ints(args.m):
        vs, cs, var = M.golomb_ruler(m, LENGTH[m])
        V = len(vs)
        ctx.set_model(V, cs.lower(V))
        lb0, ub0 = vs.bounds()
        searches = {b: DeviceSearch(ctx, batch=b, capacity=max(64 * b, 1 << 14), implicit=True, objective=(var, "min")) for b in ints(args.batch)}
        if warm:  # first launches of every kernel (code objects loaded, buffers allocated)
            forest_bnb(ctx, lb0, ub0, (var, "min"), n_trees=64, steps_per_launch=args.steps, small=True)
            for ds in searches.values():
                ds.run(lb0, ub0, node_limit=4096)
            ctx.dfs_device(lb0, ub0, 64, capacity=256, stop_on_solution=False, node_limit=64)
            warm = False
        for trees in ints(args.trees):
            r, dt = clock(lambda: forest_bnb(ctx, lb0, ub0, (var, "min"), n_trees=trees, steps_per_launch=args.steps, small=True))
            emit(m, "forest", trees, r["best"], r["nodes"], dt, trees=r["trees"], launches=r["launches"], steals=r["steals"], seeded_nodes=r["seeded_nodes"], error=r["error"])
        for b, ds in searches.items():
            st, dt = clock(lambda: ds.run(lb0, ub0))
            emit(m, "device_search", b, st.best, st.num_nodes, dt, rounds=st.rounds)
        if args.dfs_nodes:
            r, dt = clock(lambda: ctx.dfs_device(lb0, ub0, args.dfs_nodes, capacity=1024, stop_on_solution=False, node_limit=args.dfs_nodes))
            emit(m, "dfs_device", 1, None, r["nodes"], dt)
    ctx.close()


if __name__ == "__main__":
    main()
