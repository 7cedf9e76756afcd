#!/usr/bin/env python
"""Enumerate over IntervalSet<i32> domains (FDSpace) on N-queens n, one GPU, three legs in one process, nodes per second each:
  1. the forest (pcp_dfs_forest_device_set_enum: one tree per workgroup, node in LDS, undo trail) under Enumerate/MinVal and Enumerate/MiddleVal,
     the frontier expanded by pcp_branch_device_set_enum under the same distributor (search_forest.forest_search_set);
  2. the same forest under BinarySplit (pcp_dfs_forest_device_set);
  3. the host-stepped batched search (search.dfs_enumerate_set: propagate_set per batch, the numpy brancher) at batch 1 and 64.
usage: enum_set_search.py [n] [forest budget] [host budget] [trees]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import pcp_amd.engine as E
from pcp_amd import model as M
from pcp_amd import search as S
from pcp_amd.search_forest import forest_search_set

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
budget = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
host_budget = int(sys.argv[3]) if len(sys.argv) > 3 else 2_000
trees = int(sys.argv[4]) if len(sys.argv) > 4 else 512
sw = (n + 63) // 64
ctx = E.Context(0)
ctx.set_model(n, M.nqueens_props(n), set_words=sw)
ctx.set_hull(1, n)
lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)


def timed(what, run, warm):
    warm()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nodes, failed, sols = (r["nodes"], r["failed"], r["solutions"]) if isinstance(r, dict) else (r.num_nodes, r.num_failed_node, r.num_solution)
    extra = f" trees {r['trees']} seeded {r['seeded_nodes']} launches {r['launches']} error {r['error']}" if isinstance(r, dict) else f" launches {r.launches}"
    print(f"n={n} {what}: {nodes} nodes in {dt * 1e3:.1f} ms = {nodes / dt:.3e} nodes/s; failed {failed} solutions {sols}{extra}", flush=True)


for brancher, val in (("enumerate", "min"), ("enumerate", "middle"), ("split", "middle")):
    kw = dict(n_trees=trees, brancher=brancher, val=val)
    name = "forest Enumerate/" + {"min": "MinVal", "middle": "MiddleVal"}[val] if brancher == "enumerate" else "forest BinarySplit/MiddleVal"
    timed(name, lambda: forest_search_set(ctx, lb0, ub0, 1, node_limit=budget, steps_per_launch=2048, **kw),
          lambda: forest_search_set(ctx, lb0, ub0, 1, node_limit=4 * trees, steps_per_launch=4, **kw))
for batch in (1, 64):
    for val in ("min", "middle"):
        timed(f"dfs_enumerate_set batch {batch} Enumerate/{'MinVal' if val == 'min' else 'MiddleVal'}",
              lambda: S.dfs_enumerate_set(ctx, lb0, ub0, 1, all_solutions=True, node_limit=host_budget, batch=batch, val=val),
              lambda: S.dfs_enumerate_set(ctx, lb0, ub0, 1, all_solutions=True, node_limit=2 * batch, batch=batch, val=val))
