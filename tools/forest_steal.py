#!/usr/bin/env python
"""steal="host" against steal="device" in the Interval forests, alternately in one process on one context — the shapes DESIGN.md §4.6 names as
bound by the host's steals between launches:
    queens_enum    N-queens-1000, Context.dfs_forest_enum(forest="neq") under MiddleVal and MinVal at --trees trees, on the open nodes of an
                   expansion under DeviceSearch(brancher="enumerate"), with the budget of tools/enum_neq_forest.py (--per-tree nodes per tree);
    queens_split   the same store through Context.dfs_forest (BinarySplit) at --trees trees, the same budget: the leg with deep stacks, where
                   the device has to shift thousands of 8 KB rows per steal;
    golomb         model.golomb_ruler(10) minimised in the small-store forest, search_forest.forest_bnb(small=True) at --golomb-trees trees
                   (the expansion is inside the clock there, as in tools/small_forest.py).
The N-queens expansions run once per leg, outside the clock, and both settings search the same roots.  After one warm-up of both settings
each leg runs --runs times (at least 5) per setting, host and device in turn; one JSON line per leg and setting: the median wall time and
rate with their range, every run's, launches and steals of the last run.

    python tools/forest_steal.py [--n 1000] [--trees 8192] [--golomb-m 10] [--golomb-trees 13824] [--runs 5] [--out profiles/forest_steal_measured.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bnb_golomb import LENGTH, OPTIMUM  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--trees", type=int, default=8192)
    ap.add_argument("--per-tree", type=int, default=128)
    ap.add_argument("--least", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--golomb-m", type=int, default=10)
    ap.add_argument("--golomb-trees", type=int, default=13824)
    ap.add_argument("--golomb-steps", type=int, default=512)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--legs", default="queens_enum,queens_split,golomb")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_steal_measured.jsonl"))
    args = ap.parse_args()
    runs = max(args.runs, 5)
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    import pcp_amd.engine as E
    from pcp_amd import model as M
    from pcp_amd.search_forest import forest_bnb, seed_roots_interval

    gpu = torch.cuda.get_device_name(0)
    ctx = E.Context(0)
    ctx.set_option("time_kernels", 0)  # no event pair around every launch
    out = open(args.out, "w") if args.out else None
    legs = [x for x in args.legs.split(",") if x]

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    def measure(leg, run, **more):
        """run(steal) under "host" and "device" in turn: one warm-up each, then `runs` timed runs each."""
        for steal in ("host", "device"):
            run(steal)
        secs, nodes, last = {"host": [], "device": []}, {"host": [], "device": []}, {}
        for _ in range(runs):
            for steal in ("host", "device"):
                last[steal], dt = clock(lambda: run(steal))
                secs[steal].append(dt)
                nodes[steal].append(last[steal]["nodes"])
        for steal in ("host", "device"):
            rates = [k / dt for k, dt in zip(nodes[steal], secs[steal])]
            r = last[steal]
            line = json.dumps({"gpu": gpu, "leg": leg, "steal": steal, "runs": runs, **more,
                               "seconds_median": round(statistics.median(secs[steal]), 5), "seconds_min": round(min(secs[steal]), 5), "seconds_max": round(max(secs[steal]), 5),
                               "nodes_per_s_median": round(statistics.median(rates), 1), "nodes_per_s_min": round(min(rates), 1), "nodes_per_s_max": round(max(rates), 1),
                               "seconds": [round(x, 5) for x in secs[steal]], "nodes": nodes[steal], "trees": r["trees"], "launches": r["launches"], "steals": r["steals"],
                               "error": r["error"], **({"best": r["best"]} if "best" in r else {})})
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()

    n = args.n
    if "queens_enum" in legs or "queens_split" in legs:
        ctx.set_model(n, M.nqueens_props(n))
        ctx.set_hull(1, n)  # the batched kernels of the expansions then run on packed cells, as in bench.py (the forests use int2 cells)
        lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
        budget = max(args.trees * args.per_tree, args.least)
    if "queens_enum" in legs:
        for val in ("middle", "min"):
            rl, ru, _, lists = seed_roots_interval(ctx, lb0, ub0, args.trees, brancher="enumerate", val=val)
            cap = min(budget // rl.shape[0] + 64, 2048)
            measure("queens_enum", lambda steal: ctx.dfs_forest_enum(rl, ru, val=val, root_excl=lists, node_budget=budget, steps_per_launch=args.steps, capacity=cap,
                                                                    max_capacity=4096, forest="neq", steal=steal),
                    n=n, val=val, budget=budget, steps_per_launch=args.steps)
            del rl, ru, lists
    if "queens_split" in legs:
        rl, ru, _ = seed_roots_interval(ctx, lb0, ub0, args.trees)
        cap = min(budget // rl.shape[0] + 64, 2048)
        measure("queens_split", lambda steal: ctx.dfs_forest(rl, ru, node_budget=budget, steps_per_launch=args.steps, capacity=cap, max_capacity=4096, steal=steal),
                n=n, val="middle", budget=budget, steps_per_launch=args.steps)
        del rl, ru
    if "golomb" in legs:
        m = args.golomb_m
        vs, cs, var = M.golomb_ruler(m, LENGTH[m])
        V = len(vs)
        ctx.set_model(V, cs.lower(V))
        glb, gub = vs.bounds()
        measure("golomb", lambda steal: forest_bnb(ctx, glb, gub, (var, "min"), n_trees=args.golomb_trees, steps_per_launch=args.golomb_steps, small=True, steal=steal),
                m=m, length=LENGTH[m], expected=OPTIMUM[m], steps_per_launch=args.golomb_steps)
    ctx.close()


if __name__ == "__main__":
    main()
