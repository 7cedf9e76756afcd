#!/usr/bin/env python
"""Branch and bound on the shortest Golomb ruler (model.golomb_ruler: minimise the last mark) with the device-resident search
(DeviceSearch(objective=...): pcp_propagate_device_bnb + pcp_branch_device per round).  One JSON line per (m, batch): the optimum, nodes,
rounds, improvements, seconds to the end of the search, nodes/s.
usage: bnb_golomb.py [m:batch ...]   (default: 8:1 8:256 8:4096 9:1 9:256 9:4096 10:256 10:4096 — batch 1 at m = 10 is 368 487 rounds)"""
import json
import os
import sys
import time


sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pcp_amd.engine as E  # noqa: E402
from pcp_amd import model as M  # noqa: E402
from pcp_amd.search_device import DeviceSearch  # noqa: E402

LENGTH = {5: 20, 6: 30, 7: 40, 8: 50, 9: 60, 10: 80}  # the domain of the marks: [0, LENGTH[m]]
OPTIMUM = {5: 11, 6: 17, 7: 25, 8: 34, 9: 44, 10: 55}
DEFAULT = ["8:1", "8:256", "8:4096", "9:1", "9:256", "9:4096", "10:256", "10:4096"]


def run(m: int, batch: int, warm: bool = True) -> dict:
    vs, cs, var = M.golomb_ruler(m, LENGTH[m])
    V = len(vs)
    ctx = E.Context(0)
    ctx.set_model(V, cs.lower(V))
    ctx.set_option("time_kernels", 0)  # no event pair around every fixpoint launch: a round is its kernels and one copy of the counts
    lb0, ub0 = vs.bounds()
    ds = DeviceSearch(ctx, batch=batch, capacity=max(64 * batch, 1 << 14), implicit=True, objective=(var, "min"))
    if warm:
        ds.run(lb0, ub0, node_limit=4 * batch)  # first launches of every kernel (code objects loaded, buffers allocated)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = ds.run(lb0, ub0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sol = st.best_solution
    return {"m": m, "length": LENGTH[m], "batch": batch, "optimum": st.best, "expected": OPTIMUM[m], "ok": st.best == OPTIMUM[m],
            "ruler": None if sol is None else [int(x) for x in sol[:m]], "nodes": st.num_nodes, "failed": st.num_failed_node,
            "solutions": st.num_solution, "improvements": len(st.incumbents), "incumbents": st.incumbents, "rounds": st.rounds,
            "max_open": st.max_open, "seconds": round(dt, 4), "nodes_per_s": round(st.num_nodes / dt, 1)}


if __name__ == "__main__":
    cases = sys.argv[1:] or DEFAULT
    for c in cases:
        m, b = (int(x) for x in c.split(":"))
        print(json.dumps(run(m, b)), flush=True)
