"""Branch and bound over FDSpace, both engines on one set-mode context: golomb_ruler(m, length) minimised by the forest
(search_forest.forest_bnb_set: one tree per workgroup, the node in LDS, the incumbent one device word folded on node entry,
pcp_dfs_forest_device_set_bnb) and by the batched search (DeviceSearch(objective=...): pcp_propagate_device_bnb + pcp_branch_device_set, a
full row per open node in HBM).  One warm-up run of each, then the faster of two runs.  Prints one JSON line: nodes, seconds and nodes/s of
both.  The two searches visit different trees (the order in which incumbents are found differs), so the node counts are not comparable one
to one; both must return the same optimum.

    python tools/bnb_forest.py [--m 8] [--length 50] [--trees 256] [--ramp 16] [--steps 2048] [--batch 1024] [--brancher split] [--val middle]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8)
    ap.add_argument("--length", type=int, default=50)
    ap.add_argument("--trees", type=int, default=256)
    ap.add_argument("--ramp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=2048)
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
    from pcp_amd.search_forest import forest_bnb_set

    vs, cs, var = M.golomb_ruler(args.m, args.length)
    V = len(vs)
    lb0, ub0 = vs.bounds()
    base, top = int(np.min(lb0)), int(np.max(ub0))
    sw = (top - base) // 64 + 1
    ctx = E.Context(0)
    ctx.set_model(V, cs.lower(V), set_words=sw)
    ctx.set_hull(base, top)

    def forest():
        return forest_bnb_set(ctx, lb0, ub0, base, (var, "min"), n_trees=args.trees, ramp_steps=args.ramp, steps_per_launch=args.steps,
                              brancher=args.brancher, val=args.val)

    ds = DeviceSearch(ctx, batch=args.batch, capacity=64 * args.batch + 4096, implicit=True, objective=(var, "min"))

    def batched():
        return ds.run(lb0, ub0, base=base)

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

    f, t_f = timed(forest)
    d, t_d = timed(batched)
    assert f["error"] == 0 and f["best"] == d.best, (f["error"], f["best"], d.best)
    out = {"tool": "bnb_forest", "workload": f"golomb_ruler({args.m}, {args.length})", "set_words": sw, "n_vars": V, "gpu": torch.cuda.get_device_name(0),
           "optimum": f["best"],
           "forest": {"n_trees": args.trees, "ramp_steps": args.ramp, "steps_per_launch": args.steps, "brancher": args.brancher, "nodes": f["nodes"],
                      "failed": f["failed"], "solutions": f["solutions"], "splits": f["splits"], "launches": f["launches"], "seconds": round(t_f, 5),
                      "nodes_per_s": round(f["nodes"] / t_f, 1)},
           "device_search": {"batch": args.batch, "nodes": d.num_nodes, "failed": d.num_failed_node, "solutions": d.num_solution, "rounds": d.rounds,
                             "seconds": round(t_d, 5), "nodes_per_s": round(d.num_nodes / t_d, 1)}}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
