#!/usr/bin/env python
"""One solution of the reference's robot scheduling example (example/src/robot.rs; model.robot_scheduling, Interval mode) under
Brancher<InputOrder, MinVal, Enumerate> — the brancher the example writes down — against Brancher<FirstSmallestVar, MinVal, Enumerate>, on
every path the device offers for a store with formula units, in one process on one context:
    device_search  DeviceSearch(brancher="enumerate", val="min") at each --batch;
    forest         Context.dfs_forest_enum (pcp_dfs_forest_device_form_enum) with one tree, and with --trees trees seeded by
                   search_forest.seed_roots_interval, both stopping at the first solution;
    host           search.dfs_enumerate: the host-stepped loop over the same context.
Cases: --robots 2,3,4 with max_time 500 per robot beyond the first (500, 1000, 1500).  One warm-up of every path, then --runs runs each;
one JSON line per run (nodes, failed, seconds) and one per case with the median.  Every search is bounded by --node-limit and by a wall-clock
alarm of --timeout seconds (a run that hits either is reported as such, not as a result).

    python tools/robot_search.py [--robots 2,3,4] [--batch 1,64,256] [--trees 256] [--runs 5] [--out profiles/var_select_measured.jsonl]
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Timeout(Exception):
    pass


def _alarm(signum, frame):
    raise Timeout()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="2,3,4")
    ap.add_argument("--batch", default="1,64,256")
    ap.add_argument("--trees", type=int, default=256)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--node-limit", type=int, default=200000)
    ap.add_argument("--timeout", type=int, default=60)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    import pcp_amd.engine as E
    from pcp_amd import model as M
    from pcp_amd import search as S
    from pcp_amd.search_device import DeviceSearch
    from pcp_amd.search_forest import seed_roots_interval

    ints = lambda s: [int(x) for x in s.split(",") if x]
    gpu = torch.cuda.get_device_name(0)
    ctx = E.Context(0)
    ctx.set_option("time_kernels", 0)
    out = open(args.out, "a") if args.out else None
    signal.signal(signal.SIGALRM, _alarm)

    def emit(**d):
        line = json.dumps({"tool": "robot_search", "gpu": gpu, **d})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def timed(fn):
        """(result or None on a timeout, seconds)."""
        torch.cuda.synchronize()
        signal.alarm(args.timeout)
        t0 = time.perf_counter()
        try:
            r = fn()
            torch.cuda.synchronize()
        except Timeout:
            r = None
        finally:
            signal.alarm(0)
        return r, time.perf_counter() - t0

    for robots in ints(args.robots):
        max_time = 500 * max(robots - 1, 1)
        vs, cs, starts, _ = M.robot_scheduling(robots, max_time)
        M.push_model(ctx, cs, len(vs))
        lb0, ub0 = (np.ascontiguousarray(b, np.int32) for b in vs.bounds())

        def device_search(batch, sel):
            st = DeviceSearch(ctx, batch=batch, capacity=max(64 * batch, 1 << 12), implicit=True, brancher="enumerate", val="min", var_select=sel).run(
                lb0, ub0, all_solutions=False, node_limit=args.node_limit, keep_solutions=1)
            return st.num_nodes, st.num_failed_node, st.num_solution, (st.solutions[0][starts[:5]].tolist() if st.solutions else None)

        def forest(trees, sel):
            if trees == 1:
                r = ctx.dfs_forest_enum(lb0[None], ub0[None], val="min", stop_on_solution=True, want_solution=True, steps_per_launch=args.steps,
                                        node_budget=args.node_limit, var_select=sel)
                first = r["first_solutions"][0][starts[:5]].tolist() if r["solutions"] else None
                return r["nodes"], r["failed"], r["solutions"], first
            with E.var_select_scope(ctx, sel):
                rl, ru, st, lists = seed_roots_interval(ctx, lb0, ub0, trees, brancher="enumerate", val="min")
                if st.num_solution or rl.shape[0] == 0:
                    return st.num_nodes, st.num_failed_node, st.num_solution, None
                r = ctx.dfs_forest_enum(rl, ru, val="min", root_excl=lists, stop_on_solution=True, steps_per_launch=args.steps, node_budget=args.node_limit)
            return st.num_nodes + r["nodes"], st.num_failed_node + r["failed"], r["solutions"], None

        def host(sel):
            st = S.dfs_enumerate(ctx, lb0, ub0, val="min", node_limit=args.node_limit, var_select=sel)
            return st.num_nodes, st.num_failed_node, st.num_solution, (st.solutions[0][starts[:5]].tolist() if st.solutions else None)

        paths = [("device_search", b, lambda sel, b=b: device_search(b, sel)) for b in ints(args.batch)]
        paths += [("forest", t, lambda sel, t=t: forest(t, sel)) for t in (1, args.trees)]
        paths += [("host", 1, host)]
        for how, size, fn in paths:
            for sel in ("input_order", "first_smallest"):
                r, _ = timed(lambda: fn(sel))  # the warm-up: code objects loaded, buffers allocated
                secs = []
                for run in range(args.runs if r is not None else 0):
                    r, dt = timed(lambda: fn(sel))
                    if r is None:
                        break
                    secs.append(dt)
                    emit(robots=robots, max_time=max_time, n_vars=len(vs), how=how, size=size, var_select=sel, run=run, nodes=r[0], failed=r[1], solutions=r[2],
                         seconds=round(dt, 5))
                if r is None:
                    emit(robots=robots, max_time=max_time, n_vars=len(vs), how=how, size=size, var_select=sel, timeout_s=args.timeout)
                    continue
                emit(robots=robots, max_time=max_time, n_vars=len(vs), how=how, size=size, var_select=sel, runs=len(secs), nodes=r[0], failed=r[1], solutions=r[2],
                     first_starts=r[3], median_seconds=round(statistics.median(secs), 5), hit_node_limit=bool(r[2] == 0))
    ctx.close()


if __name__ == "__main__":
    main()
