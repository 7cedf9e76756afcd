"""What returning every solution costs: the same all-solutions search of an Interval forest without and with a solution sink
(search_forest.forest_search(collect_solutions=), pcp_solution_sink_set), in one process on one context, the two alternating.
  schedule   the Cumulative schedule of tools/form_forest.py (five tasks, durations 3,2,2,1,2, resources 2,1,2,1,1, capacity 3, starts 0..7)
             through the formula-store forest (pcp_dfs_forest_device_form);
  golomb6    model.golomb_ruler(6, 30) through the small-store forest under BinarySplit and under Enumerate on MinVal
             (pcp_dfs_forest_device_small, pcp_dfs_forest_device_small_enum);
  schedule6  the same with a sixth task (durations 3,2,2,1,2,1, resources 2,1,2,1,1,2): the longest of the five;
  queens8    N-queens 8 through the small-store forest under BinarySplit, 64 trees (more and the expansion finishes the tree by itself).
The variants are: no sink, and a sink of each capacity of --sink (the default pair: one that has to be drained, one that never fills).
One warm-up of each variant, then --runs timed runs of each, alternating; a run with a sink must leave the counters of the run without one
and as many rows as solutions.  Every run is one JSON line — nodes, solutions, seconds, launches, drains, rows — appended to --out; the last
lines per workload are the summaries: the median seconds without and with that sink, and their ratio.

    python tools/forest_solutions.py [--runs 7] [--trees 1024] [--steps 512] [--sink 4096,262144] [--out profiles/forest_sink_measured.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--trees", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--sink", default="4096,262144")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "forest_sink_measured.jsonl"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    import pcp_amd.engine as E
    from pcp_amd import model as M
    from pcp_amd.search_forest import forest_search
    from form_forest import schedule

    gpu = torch.cuda.get_device_name(0)
    ctx = E.Context(0)
    sinks = [int(x) for x in args.sink.split(",")]
    out = open(args.out, "a")

    def emit(**rec):
        line = json.dumps({"tool": "forest_solutions", "gpu": gpu, **rec})
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def models():
        vs, cs, _ = schedule((3, 2, 2, 1, 2), (2, 1, 2, 1, 1), 7, 0)
        yield "cumulative(3,2,2,1,2 / 2,1,2,1,1 / 3, starts 0..7)", vs, cs, dict(formulas=True)
        vs, cs, _ = schedule((3, 2, 2, 1, 2, 1), (2, 1, 2, 1, 1, 2), 7, 0)
        yield "cumulative(3,2,2,1,2,1 / 2,1,2,1,1,2 / 3, starts 0..7)", vs, cs, dict(formulas=True)
        vs, cs, _ = M.golomb_ruler(6, 30)
        yield "golomb_ruler(6, 30), BinarySplit", vs, cs, dict(small=True)
        yield "golomb_ruler(6, 30), Enumerate on MinVal", vs, cs, dict(small=True, brancher="enumerate", val="min")
        vs, cs = M.nqueens(8)
        yield "nqueens(8), BinarySplit, 64 trees", vs, cs, dict(small=True, n_trees=64)

    for work, vs, cs, kw in models():
        lb0, ub0 = vs.bounds()
        M.push_model(ctx, cs, len(vs))

        def run(sink):
            info = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = forest_search(ctx, lb0, ub0, steps_per_launch=args.steps, info=info,
                              **(dict(collect_solutions=True, sink_capacity=sink) if sink else {}), **{"n_trees": args.trees, **kw})
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
                rows = len(r["solutions_lb"]) if sink else 0
                assert not sink or rows == r["solutions"], (rows, r["solutions"])
                times[sink].append(t)
                emit(workload=work, sink=bool(sink), run=i, nodes=r["nodes"], solutions=r["solutions"], failed=r["failed"], seconds=round(t, 5),
                     nodes_per_s=round(r["nodes"] / t, 1), launches=r["launches"], drains=info.get("drains", 0), rows=rows, n_trees=r["trees"],
                     steps_per_launch=args.steps, sink_capacity=sink)
        assert len(counters) == 1, counters
        med = {k: statistics.median(v) for k, v in times.items()}
        for sink in sinks:
            emit(workload=work, summary=True, runs=args.runs, sink_capacity=sink, median_seconds_without=round(med[0], 5), median_seconds_with=round(med[sink], 5),
                 ratio=round(med[sink] / med[0], 3), min_seconds_without=round(min(times[0]), 5), min_seconds_with=round(min(times[sink]), 5))
    out.close()
    ctx.close()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
