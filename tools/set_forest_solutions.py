"""What returning every solution costs in set mode: the same all-solutions search of a set-mode forest without and with a set solution sink
(search_forest.forest_search_set(collect_solutions=), pcp_set_solution_sink_set), in one process on one context, the variants alternating —
the set-mode twin of tools/forest_solutions.py.
  queens8    N-queens 8 over sets through the records forest (pcp_dfs_forest_device_set), under BinarySplit and under Enumerate on MinVal;
  sched4     the four-task schedule of tests/setform_forest_ref.py (durations 2,3,2,1) through the formula forest (pcp_dfs_forest_device_setform);
  sched5     its five-task schedule (durations 3,2,4,2,3).
The variants are: no sink, a sink that never fills, and a small sink that must be drained (--sink: the two capacities).  One warm-up of each
variant, then --runs timed runs of each, alternating; a run with a sink must leave the counters of the run without one and as many rows as
solutions.  Every run is one JSON line — nodes, solutions, seconds, launches, drains, rows — appended to --out; the last lines per workload
are the summaries: the median seconds without and with that sink, and their ratio.  No ratio is fixed in advance.

    python tools/set_forest_solutions.py [--runs 7] [--trees 64] [--steps 256] [--horizon 16] [--sink 65536,64] [--out profiles/set_forest_sink_measured.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--trees", type=int, default=64)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--sink", default="65536,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_forest_sink_measured.jsonl"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import pcp_amd.engine as E
    from pcp_amd import model as M
    from pcp_amd.search_forest import forest_search_set
    import setform_forest_ref as R

    gpu = torch.cuda.get_device_name(0)
    ctx = E.Context(0)
    sinks = [int(x) for x in args.sink.split(",")]
    out = open(args.out, "a")

    def emit(**rec):
        line = json.dumps({"tool": "set_forest_solutions", "gpu": gpu, **rec})
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def models():
        vs, cs = M.nqueens(8)
        yield "nqueens(8) over sets, BinarySplit", vs, cs, (1, 8), dict()
        yield "nqueens(8) over sets, Enumerate on MinVal", vs, cs, (1, 8), dict(brancher="enumerate", val="min")
        for dur in (R.DUR4, R.DUR5):
            vs, cs, _ = R.schedule(dur, args.horizon)
            yield f"disjunctive_schedule({list(dur)}, {args.horizon}), BinarySplit", vs, cs, (0, args.horizon), dict(formulas=True)

    for work, vs, cs, hull, kw in models():
        lb0, ub0 = vs.bounds()
        M.push_model(ctx, cs, len(vs), 1)
        ctx.set_hull(*hull)

        def run(sink):
            info = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = forest_search_set(ctx, lb0, ub0, hull[0], n_trees=args.trees, steps_per_launch=args.steps, info=info,
                                  **(dict(collect_solutions=True, sink_capacity=sink) if sink else {}), **kw)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            assert r["error"] == 0, r
            return r, t, info

        variants = [0] + sinks  # 0: no sink
        for sink in variants:  # warm-up: allocations, the first launch of every kernel
            run(sink)
        times = {v: [] for v in variants}
        counters = set()
        for i in range(args.runs):
            for sink in variants:
                r, t, info = run(sink)
                counters.add((r["nodes"], r["solutions"], r["failed"]))
                rows = len(r["solutions_bits"]) if sink else 0
                assert not sink or rows == r["solutions"], (rows, r["solutions"])
                times[sink].append(t)
                emit(workload=work, sink=bool(sink), run=i, nodes=r["nodes"], solutions=r["solutions"], failed=r["failed"], seconds=round(t, 5),
                     nodes_per_s=round(r["nodes"] / t, 1), launches=r["launches"], drains=info.get("drains", 0), handed_back=info.get("handed_back", 0),
                     rows=rows, n_trees=r["trees"], steps_per_launch=args.steps, sink_capacity=sink)
        assert len(counters) == 1, counters
        med = {k: statistics.median(v) for k, v in times.items()}
        for sink in sinks:
            emit(workload=work, summary=True, runs=args.runs, sink_capacity=sink, median_seconds_without=round(med[0], 5), median_seconds_with=round(med[sink], 5),
                 ratio=round(med[sink] / med[0], 3), min_seconds_without=round(min(times[0]), 5), min_seconds_with=round(min(times[sink]), 5),
                 max_seconds_without=round(max(times[0]), 5), max_seconds_with=round(max(times[sink]), 5))
    out.close()
    ctx.close()


if __name__ == "__main__":
    main()
