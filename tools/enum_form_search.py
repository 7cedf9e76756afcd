#!/usr/bin/env python
"""A makespan schedule (five tasks under propagators::Cumulative: durations 3,2,4,1,2, resources 2,1,2,1,1, capacity 3, starts 0..8, a makespan
variable 0..14 — tools/form_forest.py's) solved to its optimum and its proof on the device-resident search, three ways in one process on one
context: DeviceSearch(brancher="enumerate", objective=...) under MinVal and under MiddleVal — pcp_propagate_device_form_excl +
pcp_branch_device_excl per round — and DeviceSearch(objective=...) under BinarySplit (pcp_propagate_device_bnb + pcp_branch_device) at the same
batch.  search.dfs_enumerate(objective=...), the host-stepped specification of the Enumerate searches (the same nodes, every batch crossing
PCIe), runs in the same process as the baseline.  One JSON line per (batch, search): the optimum, nodes, rounds, improvements, seconds to the end
of the search, nodes/s — one run each after a warm-up, as measured.  The three distributors visit three different trees.
usage: enum_form_search.py [batch ...]   (default: 64 256)"""
import json
import os
import sys
import time


sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pcp_amd.engine as E  # noqa: E402
from pcp_amd import model as M  # noqa: E402
from pcp_amd import search as S  # noqa: E402
from pcp_amd.search_device import DeviceSearch  # noqa: E402

DURATIONS, RESOURCES, CAPACITY, HORIZON, MAKESPAN, OPTIMUM = (3, 2, 4, 1, 2), (2, 1, 2, 1, 1), 3, 8, 14, 7
SEARCHES = [("device", "enumerate", "min"), ("device", "enumerate", "middle"), ("device", "split", "middle"), ("host", "enumerate", "min"), ("host", "enumerate", "middle")]


def schedule():
    vs, cs = M.VStore(), M.CStore()
    s = [vs.alloc((0, HORIZON)) for _ in DURATIONS]
    mk = vs.alloc((0, MAKESPAN))
    cap = vs.alloc((CAPACITY, CAPACITY))
    M.Cumulative(s, [M.Constant(d) for d in DURATIONS], [M.Constant(r) for r in RESOURCES], cap).join(vs, cs)
    for si, d in zip(s, DURATIONS):
        cs.alloc(M.x_leq_y(M.Addition(si, d), mk))
    return vs, cs, mk.idx


def run(ctx, batch: int, driver: str, brancher: str, val: str, lb0, ub0, var) -> dict:
    if driver == "device":
        ds = DeviceSearch(ctx, batch=batch, capacity=max(64 * batch, 1 << 14), implicit=True, objective=(var, "min"), brancher=brancher, val=val)
        go = lambda limit=0: ds.run(lb0, ub0, node_limit=limit)
    else:
        go = lambda limit=0: S.dfs_enumerate(ctx, lb0, ub0, batch=batch, val=val, objective=(var, "min"), node_limit=limit)
    go(4 * batch)  # first launches of every kernel (code objects loaded, buffers allocated)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = go()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sol = st.best_solution
    return {"tool": "enum_form_search", "tasks": len(DURATIONS), "batch": batch, "driver": "DeviceSearch" if driver == "device" else "dfs_enumerate",
            "brancher": brancher, "val": val if brancher == "enumerate" else None, "optimum": st.best, "expected": OPTIMUM, "ok": st.best == OPTIMUM,
            "starts": None if sol is None else [int(x) for x in sol[:len(DURATIONS)]], "nodes": st.num_nodes, "failed": st.num_failed_node,
            "solutions": st.num_solution, "improvements": len(st.incumbents), "rounds": getattr(st, "rounds", None) or getattr(st, "launches", None),
            "path": ctx.last_plan()["path"], "seconds": round(dt, 4), "nodes_per_s": round(st.num_nodes / dt, 1)}


if __name__ == "__main__":
    vs, cs, var = schedule()
    ctx = E.Context(0)
    M.push_model(ctx, cs, len(vs))
    ctx.set_option("time_kernels", 0)  # no event pair around every fixpoint launch: a round is its kernels and one copy of the counts
    lb0, ub0 = vs.bounds()
    for b in [int(x) for x in sys.argv[1:]] or [64, 256]:
        for driver, brancher, val in SEARCHES:
            print(json.dumps(run(ctx, b, driver, brancher, val, lb0, ub0, var)), flush=True)
    ctx.close()
