#!/usr/bin/env python
"""Enumerate in the all-XNeqY in-kernel forest (pcp_dfs_forest_device_neq_enum) on N-queens-1000, against the batched Enumerate search and
against the BinarySplit forest, all in one process on one context, under MiddleVal and MinVal, each case with a fixed node budget:
    enum_forest    Context.dfs_forest_enum(forest="neq") on the open nodes of an expansion under DeviceSearch(brancher="enumerate") — each
                   root with the exclusion list the expansion gave it — at each number of --trees: one workgroup per tree, one exclusion
                   path per tree, nothing copied at a branch;
    enum_search    DeviceSearch(brancher="enumerate", val=) at --batch: a CSR list per open node, copied and filtered at every branch
                   (pcp_propagate_device_excl + pcp_branch_device_excl);
    split_forest   Context.dfs_forest — the same kernel's loop under BinarySplit — on the open nodes of a BinarySplit expansion, at each
                   number of --trees.
The forests' clocks cover the launches of the trees (the expansion is run once per case, outside the clock, and its roots are reused); the
budget of a forest is --per-tree nodes per tree, at least --least, checked between launches, so a run counts a little more — the rate is
nodes counted over seconds.  After one warm-up of every entry each case runs --runs times (at least 5); one JSON line per case: the median
rate, the lowest and the highest, every run's.  The trees of the three differ (distributor, order), so the lines compare rates, not nodes.

    python tools/enum_neq_forest.py [--n 1000] [--trees 1,256,8192] [--batch 1024] [--runs 5] [--out profiles/enum_neq_forest_measured.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--trees", default="1,256,8192")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--per-tree", type=int, default=128)
    ap.add_argument("--least", type=int, default=16384)
    ap.add_argument("--search-nodes", type=int, default=1 << 18)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enum_neq_forest_measured.jsonl"))
    args = ap.parse_args()
    runs = max(args.runs, 5)
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    import pcp_amd.engine as E
    from pcp_amd import model as M
    from pcp_amd.search_device import DeviceSearch
    from pcp_amd.search_forest import seed_roots_interval

    n = args.n
    gpu = torch.cuda.get_device_name(0)
    ctx = E.Context(0)
    ctx.set_option("time_kernels", 0)  # no event pair around every launch
    ctx.set_model(n, M.nqueens_props(n))
    ctx.set_hull(1, n)  # the batched kernels of the expansions and of enum_search then run on packed cells, as in bench.py (the forests use int2 cells)
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    out = open(args.out, "w") if args.out else None

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    def emit(how, val, size, budget, rates, nodes, **more):
        line = json.dumps({"gpu": gpu, "n": n, "how": how, "val": val, "size": size, "budget": budget, "runs": len(rates),
                           "nodes_per_s_median": round(statistics.median(rates), 1), "nodes_per_s_min": round(min(rates), 1), "nodes_per_s_max": round(max(rates), 1),
                           "nodes_per_s": [round(x, 1) for x in rates], "nodes": nodes, **more})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def budget_of(trees):
        return max(trees * args.per_tree, args.least)

    def steps_of(n_trees):  # (one tree alone: long launches, or the clock measures the host's loop)
        return 1024 if n_trees == 1 else args.steps

    def enum_forest(roots, val, budget):
        rl, ru, lists = roots
        cap = min(budget // rl.shape[0] + 64, 2048)
        return ctx.dfs_forest_enum(rl, ru, val=val, root_excl=lists, node_budget=budget, steps_per_launch=steps_of(rl.shape[0]), capacity=cap, max_capacity=4096, forest="neq")

    def split_forest(roots, budget):
        rl, ru = roots
        cap = min(budget // rl.shape[0] + 64, 2048)
        return ctx.dfs_forest(rl, ru, node_budget=budget, steps_per_launch=steps_of(rl.shape[0]), capacity=cap, max_capacity=4096)

    def enum_roots(trees, val):
        if trees == 1:
            return torch.from_numpy(lb0[None]).cuda(), torch.from_numpy(ub0[None]).cuda(), None
        rl, ru, _, lists = seed_roots_interval(ctx, lb0, ub0, trees, brancher="enumerate", val=val)
        return rl, ru, lists

    def split_roots(trees):
        if trees == 1:
            return torch.from_numpy(lb0[None]).cuda(), torch.from_numpy(ub0[None]).cuda()
        rl, ru, _ = seed_roots_interval(ctx, lb0, ub0, trees)
        return rl, ru

    # (a node leaves at most one more open node behind than it took: the stack never holds more rows than the budget plus the first batches')
    search = lambda val: DeviceSearch(ctx, batch=args.batch, capacity=args.search_nodes + 64 * args.batch, implicit=True, brancher="enumerate", val=val)
    tree_counts = [int(x) for x in args.trees.split(",") if x]
    # warm-up: the first launches of every kernel (code objects loaded, allocator warmed)
    for val in ("middle", "min"):
        enum_forest(enum_roots(64, val), val, 4096)
        search(val).run(lb0, ub0, node_limit=4096)
    split_forest(split_roots(64), 4096)

    def measure(fn):
        rates, nodes, last = [], [], None
        for _ in range(runs):
            last, dt = clock(fn)
            k = last["nodes"] if isinstance(last, dict) else last.num_nodes
            rates.append(k / dt)
            nodes.append(k)
        return rates, nodes, last

    for val in ("middle", "min"):
        for trees in tree_counts:
            roots, budget = enum_roots(trees, val), budget_of(trees)
            rates, nodes, r = measure(lambda: enum_forest(roots, val, budget))
            emit("enum_forest", val, trees, budget, rates, nodes, trees=r["trees"], launches=r["launches"], steals=r["steals"], error=r["error"], steps_per_launch=steps_of(r["trees"]))
            del roots
        ds = search(val)
        rates, nodes, st = measure(lambda: ds.run(lb0, ub0, node_limit=args.search_nodes))
        emit("enum_search", val, args.batch, args.search_nodes, rates, nodes)
        del ds
    for trees in tree_counts:
        roots, budget = split_roots(trees), budget_of(trees)
        rates, nodes, r = measure(lambda: split_forest(roots, budget))
        emit("split_forest", "middle", trees, budget, rates, nodes, trees=r["trees"], launches=r["launches"], steals=r["steals"], error=r["error"], steps_per_launch=steps_of(r["trees"]))
        del roots
    ctx.close()


if __name__ == "__main__":
    main()
