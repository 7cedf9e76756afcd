#!/usr/bin/env python
"""The shortest Golomb ruler (model.golomb_ruler: minimise the last mark) under Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate> with
the device-resident search: DeviceSearch(brancher="enumerate", objective=...) — pcp_propagate_device_small_excl + pcp_branch_device_excl per
round —, beside DeviceSearch(objective=...) under BinarySplit (pcp_propagate_device_bnb + pcp_branch_device) at the same batch, in the same
process.  One JSON line per (m, batch, brancher): the optimum, nodes, rounds, improvements, seconds to the end of the search (the optimum and
its proof), nodes/s — one run each, as measured.  Enumerate visits another tree than BinarySplit: the node counts differ by design.
Set mode is not measured: DeviceSearch takes no objective under Enumerate there (search_forest.forest_bnb_set is that column), and the tree of
all solutions of these models is not a search anybody runs.
usage: enum_small_search.py [m:batch ...]   (default: 8:256 9:256 10:256)"""
import json
import os
import sys
import time


sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pcp_amd.engine as E  # noqa: E402
from pcp_amd import model as M  # noqa: E402
from pcp_amd.search_device import DeviceSearch  # noqa: E402

LENGTH = {5: 20, 6: 30, 7: 40, 8: 50, 9: 60, 10: 80}  # the domain of the marks: [0, LENGTH[m]] (tools/bnb_golomb.py)
OPTIMUM = {5: 11, 6: 17, 7: 25, 8: 34, 9: 44, 10: 55}
DEFAULT = ["8:256", "9:256", "10:256"]
BRANCHERS = [("enumerate", "middle"), ("enumerate", "min"), ("split", "middle")]


def run(ctx, m: int, batch: int, brancher: str, val: str, lb0, ub0, var) -> dict:
    ds = DeviceSearch(ctx, batch=batch, capacity=max(64 * batch, 1 << 14), implicit=True, objective=(var, "min"), brancher=brancher, val=val)
    ds.run(lb0, ub0, node_limit=4 * batch)  # first launches of every kernel (code objects loaded, buffers allocated)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = ds.run(lb0, ub0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sol = st.best_solution
    return {"m": m, "length": LENGTH[m], "batch": batch, "brancher": brancher, "val": val if brancher == "enumerate" else None, "optimum": st.best,
            "expected": OPTIMUM[m], "ok": st.best == OPTIMUM[m], "ruler": None if sol is None else [int(x) for x in sol[:m]], "nodes": st.num_nodes,
            "failed": st.num_failed_node, "solutions": st.num_solution, "improvements": len(st.incumbents), "rounds": st.rounds, "max_open": st.max_open,
            "path": ctx.last_plan()["path"], "seconds": round(dt, 4), "nodes_per_s": round(st.num_nodes / dt, 1)}


if __name__ == "__main__":
    for c in sys.argv[1:] or DEFAULT:
        m, b = (int(x) for x in c.split(":"))
        vs, cs, var = M.golomb_ruler(m, LENGTH[m])
        ctx = E.Context(0)
        ctx.set_model(len(vs), cs.lower(len(vs)))
        ctx.set_option("time_kernels", 0)  # no event pair around every fixpoint launch: a round is its kernels and one copy of the counts
        lb0, ub0 = vs.bounds()
        for brancher, val in BRANCHERS:
            print(json.dumps(run(ctx, m, b, brancher, val, lb0, ub0, var)), flush=True)
        ctx.close()
