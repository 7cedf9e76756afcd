"""Enumerate at scale, both halves on the device: N-queens-n (declared hull) under Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate>
and one node budget, searched by the host-stepped loop (search.dfs_enumerate: rows to the host, numpy brancher, CSR rebuilt and uploaded every
round) and by DeviceSearch(brancher="enumerate") (rows, hints and exclusion lists stay on the GPU; eight counters cross PCIe per round), in one
process on one GPU.  Prints one JSON line: nodes/s and rounds of both, the speed-up, and the brancher's share of the device loop's kernel time
(HIP events around every propagate / branch call of the round).

    python tools/enum_search.py [--n 1000] [--nodes 8192] [--batches 64,1024] [--vals middle,min]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class TimedCtx:
    """The context with HIP events around the two calls of an Enumerate round (everything else is forwarded)."""

    def __init__(self, ctx, torch):
        self._ctx, self._torch, self.events = ctx, torch, {"propagate": [], "branch": []}

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def _timed(self, kind, fn, *a, **kw):
        e0, e1 = self._torch.cuda.Event(enable_timing=True), self._torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(*a, **kw)
        e1.record()
        self.events[kind].append((e0, e1))

    def propagate_device_excl(self, *a, **kw):
        self._timed("propagate", self._ctx.propagate_device_excl, *a, **kw)

    def branch_device_excl(self, *a, **kw):
        self._timed("branch", self._ctx.branch_device_excl, *a, **kw)

    def ms(self, kind):
        return sum(a.elapsed_time(b) for a, b in self.events[kind])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--nodes", type=int, default=8192)
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--vals", default="middle,min")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import pcp_amd.engine as E
    from pcp_amd import model as M
    from pcp_amd import search as S
    from pcp_amd.search_device import DeviceSearch

    n = args.n
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    ctx = E.Context(0)
    ctx.set_model(n, M.nqueens_props(n))
    ctx.set_hull(1, n)
    out = {"tool": "enum_search", "workload": f"nqueens-{n}", "node_budget": args.nodes, "gpu": torch.cuda.get_device_name(0), "runs": []}
    for val in args.vals.split(","):
        for batch in (int(b) for b in args.batches.split(",")):
            # (Enumerate's tree is deep — a level per value —: the stack is sized by the budget, one node visited leaves at most one more open)
            cap = 2 * args.nodes + 2 * batch + 64
            ds = DeviceSearch(ctx, batch=batch, capacity=cap, implicit=True, brancher="enumerate", val=val)
            # warm-up of both loops (allocations, the first launch of every kernel)
            S.dfs_enumerate(ctx, lb0, ub0, all_solutions=True, node_limit=4 * batch, batch=batch, val=val)
            ds.run(lb0, ub0, all_solutions=True, node_limit=4 * batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = S.dfs_enumerate(ctx, lb0, ub0, all_solutions=True, node_limit=args.nodes, batch=batch, val=val)
            torch.cuda.synchronize()
            t_host = time.perf_counter() - t0
            t0 = time.perf_counter()
            dev = ds.run(lb0, ub0, all_solutions=True, node_limit=args.nodes)
            torch.cuda.synchronize()
            t_dev = time.perf_counter() - t0
            # (both visit `nodes` nodes; with batch > 1 the two loops take a round's open nodes in opposite order, so under a budget they need not
            # be the same nodes: the whole trees are equal, tests/test_branch_excl.py)
            counts = {"host": [host.num_nodes, host.num_solution, host.num_failed_node], "device": [dev.num_nodes, dev.num_solution, dev.num_failed_node]}
            # the same device loop once more under events: the brancher's share of the kernel time
            timed = TimedCtx(ctx, torch)
            ds_t = DeviceSearch(timed, batch=batch, capacity=cap, implicit=True, brancher="enumerate", val=val)
            ds_t.run(lb0, ub0, all_solutions=True, node_limit=args.nodes)
            torch.cuda.synchronize()
            p_ms, b_ms = timed.ms("propagate"), timed.ms("branch")
            out["runs"].append({"val": val, "batch": batch, "nodes_solutions_failures": counts,
                                "host_nodes_per_s": round(host.num_nodes / t_host, 1), "host_rounds": host.launches,
                                "device_nodes_per_s": round(dev.num_nodes / t_dev, 1), "device_rounds": dev.rounds,
                                "speedup": round((dev.num_nodes / t_dev) / (host.num_nodes / t_host), 2),
                                "propagate_ms": round(p_ms, 3), "branch_ms": round(b_ms, 3), "brancher_share": round(b_ms / (p_ms + b_ms), 4)})
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
