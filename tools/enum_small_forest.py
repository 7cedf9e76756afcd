#!/usr/bin/env python
"""Enumerate in the small-store forest (pcp_dfs_forest_device_small_enum) on the shortest Golomb ruler, against the batched Enumerate search
and against the BinarySplit forest, all in one process on one context: model.golomb_ruler(m, LENGTH[m]) for m = 8, 9, 10 (the lengths and
optima of tools/bnb_golomb.py), the last mark minimised.
    enum_forest    search_forest.forest_bnb(small=True, brancher="enumerate", val=) under MinVal and MiddleVal at each number of --trees: one
                   tree per wavefront, one exclusion path per tree, nothing copied at a branch;
    enum_search    DeviceSearch(brancher="enumerate", val=, objective=) at each --batch: a CSR list per open node, copied and filtered at
                   every branch (pcp_propagate_device_small_excl + pcp_branch_device_excl);
    split_forest   search_forest.forest_bnb(small=True) — the same forest under BinarySplit — at each number of --trees.
One warm-up of each entry on the first m, then every case once.  Prints one JSON line per case: optimum, nodes, seconds, nodes/s.  The
minimisations visit different trees (the incumbent arrives at different moments, and the distributors differ) and must agree on the optimum.

    python tools/enum_small_forest.py [--m 8,9,10] [--trees 256,13824] [--batch 256,4096] [--steps 512] [--out FILE]
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
    ap.add_argument("--trees", default="256,13824")
    ap.add_argument("--batch", default="256,4096")
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--out", default="")
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
    out = open(args.out, "w") if args.out else None

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    def emit(m, how, val, size, optimum, nodes, dt, **more):
        line = json.dumps({"gpu": gpu, "m": m, "length": LENGTH[m], "how": how, "val": val, "size": size, "optimum": optimum, "expected": OPTIMUM[m],
                           "ok": optimum == OPTIMUM[m], "nodes": nodes, "seconds": round(dt, 4), "nodes_per_s": round(nodes / dt, 1), **more})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def forest(lb0, ub0, var, trees, **kw):
        return forest_bnb(ctx, lb0, ub0, (var, "min"), n_trees=trees, steps_per_launch=args.steps, small=True, **kw)

    warm = True
    for m in ints(args.m):
        vs, cs, var = M.golomb_ruler(m, LENGTH[m])
        V = len(vs)
        ctx.set_model(V, cs.lower(V))
        lb0, ub0 = vs.bounds()
        search = lambda b, val: DeviceSearch(ctx, batch=b, capacity=max(64 * b, 1 << 14), implicit=True, objective=(var, "min"), brancher="enumerate", val=val)
        if warm:  # first launches of every kernel (code objects loaded, buffers allocated)
            for val in ("min", "middle"):
                forest(lb0, ub0, var, 64, brancher="enumerate", val=val)
                search(256, val).run(lb0, ub0, node_limit=4096)
            forest(lb0, ub0, var, 64)
            warm = False
        for val in ("min", "middle"):
            for trees in ints(args.trees):
                info = {}
                r, dt = clock(lambda: forest(lb0, ub0, var, trees, brancher="enumerate", val=val, info=info))
                emit(m, "enum_forest", val, trees, r["best"], r["nodes"], dt, trees=r["trees"], launches=r["launches"], steals=r["steals"],
                     seeded_nodes=r["seeded_nodes"], error=r["error"], path_capacity=info.get("path_capacity"), capacity=info.get("capacity"))
            for b in ints(args.batch):
                ds = search(b, val)
                st, dt = clock(lambda: ds.run(lb0, ub0))
                emit(m, "enum_search", val, b, st.best, st.num_nodes, dt, rounds=st.rounds)
                del ds
        for trees in ints(args.trees):
            r, dt = clock(lambda: forest(lb0, ub0, var, trees))
            emit(m, "split_forest", "middle", trees, r["best"], r["nodes"], dt, trees=r["trees"], launches=r["launches"], steals=r["steals"],
                 seeded_nodes=r["seeded_nodes"], error=r["error"])
    ctx.close()


if __name__ == "__main__":
    main()
