#!/usr/bin/env python
"""Enumerate in the formula-store forest (pcp_dfs_forest_device_form_enum) on makespan schedules, against the batched Enumerate search and
against the BinarySplit forest, all in one process on one context.  Two models of one family (tasks under propagators::Cumulative, capacity
3, a makespan variable minimised to its optimum and its proof): "five" — tools/enum_form_search.py's five tasks — and "seven", the same
five plus two, whose trees are beyond 10^5 nodes.
    enum_forest    search_forest.forest_enumerate(objective=, val=) under MinVal and MiddleVal at each number of --trees: one tree per
                   wavefront, one exclusion path per tree, nothing copied at a branch;
    enum_search    DeviceSearch(brancher="enumerate", val=, objective=) at each --batch: a CSR list per open node, copied and filtered at
                   every branch (pcp_propagate_device_form_excl + pcp_branch_device_excl);
    split_forest   search_forest.forest_bnb — the same forest under BinarySplit — at each number of --trees.
One warm-up of each entry, then every case --runs times; one JSON line per run (optimum, nodes, seconds, nodes/s, run index), appended to
--out.  The minimisations visit different trees (the incumbent arrives at different moments, and the distributors differ) and must agree
on the optimum.

    python tools/enum_form_forest.py [--models five,seven] [--trees 1,256,13824] [--batch 256,1024] [--steps 512] [--runs 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CAPACITY = 3
# name -> (durations, resources, last start, last makespan)
MODELS = {
    "five": ((3, 2, 4, 1, 2), (2, 1, 2, 1, 1), 8, 14),
    "seven": ((3, 2, 4, 1, 2, 3, 2), (2, 1, 2, 1, 1, 2, 1), 12, 20),
}


def schedule(M, name):
    durations, resources, horizon, makespan = MODELS[name]
    vs, cs = M.VStore(), M.CStore()
    s = [vs.alloc((0, horizon)) for _ in durations]
    mk = vs.alloc((0, makespan))
    cap = vs.alloc((CAPACITY, CAPACITY))
    M.Cumulative(s, [M.Constant(d) for d in durations], [M.Constant(r) for r in resources], cap).join(vs, cs)
    for si, d in zip(s, durations):
        cs.alloc(M.x_leq_y(M.Addition(si, d), mk))
    return vs, cs, mk.idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="five,seven")
    ap.add_argument("--trees", default="1,256,13824")
    ap.add_argument("--batch", default="256,1024")
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import pcp_amd.engine as E
    from pcp_amd import model as M
    from pcp_amd.search_device import DeviceSearch
    from pcp_amd.search_forest import forest_bnb, forest_enumerate

    ints = lambda s: [int(x) for x in s.split(",") if x]
    gpu = torch.cuda.get_device_name(0)
    ctx = E.Context(0)
    ctx.set_option("time_kernels", 0)  # no event pair around every launch
    out = open(args.out, "a") if args.out else None

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    def emit(model, how, val, size, run, optimum, nodes, dt, **more):
        line = json.dumps({"tool": "enum_form_forest", "gpu": gpu, "model": model, "tasks": len(MODELS[model][0]), "how": how, "val": val, "size": size, "run": run,
                           "optimum": optimum, "nodes": nodes, "seconds": round(dt, 4), "nodes_per_s": round(nodes / dt, 1), **more})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for model in [m for m in args.models.split(",") if m]:
        vs, cs, var = schedule(M, model)
        M.push_model(ctx, cs, len(vs))
        lb0, ub0 = vs.bounds()
        enum = lambda trees, val, **kw: forest_enumerate(ctx, lb0, ub0, val=val, objective=(var, "min"), n_trees=trees, steps_per_launch=args.steps, **kw)
        split = lambda trees: forest_bnb(ctx, lb0, ub0, (var, "min"), n_trees=trees, steps_per_launch=args.steps)
        search = lambda b, val: DeviceSearch(ctx, batch=b, capacity=max(64 * b, 1 << 14), implicit=True, objective=(var, "min"), brancher="enumerate", val=val)
        for val in ("min", "middle"):  # first launches of every kernel (code objects loaded, buffers allocated)
            enum(64, val)
            search(256, val).run(lb0, ub0, node_limit=4096)
        split(64)
        for val in ("min", "middle"):
            for trees in ints(args.trees):
                for run in range(args.runs):
                    info = {}
                    r, dt = clock(lambda: enum(trees, val, info=info))
                    emit(model, "enum_forest", val, trees, run, r["best"], r["nodes"], dt, trees=r["trees"], launches=r["launches"], steals=r["steals"],
                         seeded_nodes=r["seeded_nodes"], error=r["error"], path_capacity=info.get("path_capacity"), capacity=info.get("capacity"))
            for b in ints(args.batch):
                for run in range(args.runs):
                    ds = search(b, val)
                    st, dt = clock(lambda: ds.run(lb0, ub0))
                    emit(model, "enum_search", val, b, run, st.best, st.num_nodes, dt, rounds=st.rounds)
                    del ds
        for trees in ints(args.trees):
            for run in range(args.runs):
                r, dt = clock(lambda: split(trees))
                emit(model, "split_forest", "middle", trees, run, r["best"], r["nodes"], dt, trees=r["trees"], launches=r["launches"], steals=r["steals"],
                     seeded_nodes=r["seeded_nodes"], error=r["error"])
    ctx.close()


if __name__ == "__main__":
    main()
