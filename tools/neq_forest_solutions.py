"""What returning every solution costs in the all-XNeqY forest, and what it gains over the small-store forest: all solutions of N-queens 10
and 12 under BinarySplit and under Enumerate on MinVal, in one process on one context, four variants alternating —
  count        the counting entries (search_forest.forest_search / forest_enumerate(forest="neq"): pcp_dfs_forest_device, _neq_enum);
  sink_ample   search_forest.forest_solutions(forest="neq") with a sink that never fills (pcp_dfs_forest_device_neq_sink);
  sink_4096    the same with a 4 096-row sink (N-queens 12 has 14 200 solutions: it must be drained; N-queens 10 has 724: it never fills);
  small        forest_search / forest_enumerate(small=True / forest="small", collect_solutions=True): the small-store forest with the
               context's sink at its default 4 096 rows — the only other forest that returns the solutions of an N-queens store.
One warm-up of each variant, then --runs timed runs of each; every variant must leave the counters of `count`, and every variant with a
sink as many rows as solutions.  Every run is one JSON line appended to --out; the last lines per workload are the summaries: median and
min - max seconds per variant and the ratios sink / count and small / sink.  No ratio is fixed in advance.

    python tools/neq_forest_solutions.py [--runs 5] [--sizes 10,12] [--trees 512] [--steps 512] [--out profiles/neq_forest_sink_measured.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AMPLE = 1 << 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sizes", default="10,12")
    ap.add_argument("--trees", type=int, default=512)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neq_forest_sink_measured.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    import pcp_amd.engine as E
    from pcp_amd import model as M
    from pcp_amd.search_forest import forest_enumerate, forest_search, forest_solutions

    gpu = torch.cuda.get_device_name(0)
    ctx = E.Context(0)
    out = open(args.out, "a")

    def emit(**rec):
        line = json.dumps({"tool": "neq_forest_solutions", "gpu": gpu, **rec})
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for n in (int(x) for x in args.sizes.split(",")):
        vs, cs = M.nqueens(n)
        M.push_model(ctx, cs, len(vs))
        lb0, ub0 = (np.ascontiguousarray(a, np.int32) for a in vs.bounds())
        for brancher, val in (("split", "middle"), ("enumerate", "min")):
            work = f"nqueens({n}), " + ("BinarySplit" if brancher == "split" else "Enumerate on MinVal")
            common = dict(n_trees=args.trees, steps_per_launch=args.steps)

            def run(variant):
                info = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if variant == "count":
                    r = forest_search(ctx, lb0, ub0, info=info, **common) if brancher == "split" else forest_enumerate(ctx, lb0, ub0, val=val, forest="neq", info=info, **common)
                elif variant == "small":
                    r = (forest_search(ctx, lb0, ub0, small=True, collect_solutions=True, info=info, **common) if brancher == "split" else
                         forest_enumerate(ctx, lb0, ub0, val=val, forest="small", collect_solutions=True, info=info, **common))
                else:
                    r = forest_solutions(ctx, lb0, ub0, brancher=brancher, val=val, forest="neq", sink_capacity=AMPLE if variant == "sink_ample" else 4096, info=info, **common)
                torch.cuda.synchronize()
                t = time.perf_counter() - t0
                assert r["error"] == 0, r
                return r, t, info

            variants = ["count", "sink_ample", "sink_4096", "small"]
            for v in variants:  # warm-up: allocations, the first launch of every kernel
                run(v)
            times = {v: [] for v in variants}
            counters = set()
            for i in range(args.runs):
                for v in variants:
                    r, t, info = run(v)
                    counters.add((r["nodes"], r["solutions"], r["failed"]))
                    rows = len(r["solutions_lb"]) if v != "count" else 0
                    assert v == "count" or rows == r["solutions"], (v, rows, r["solutions"])
                    times[v].append(t)
                    emit(workload=work, variant=v, run=i, nodes=r["nodes"], solutions=r["solutions"], failed=r["failed"], seconds=round(t, 5),
                         nodes_per_s=round(r["nodes"] / t, 1), launches=r["launches"], drains=info.get("drains", 0), steals=info.get("steals", 0), rows=rows,
                         n_trees=r["trees"], steps_per_launch=args.steps, sink_capacity={"count": 0, "sink_ample": AMPLE}.get(v, 4096))
            assert len(counters) == 1, counters
            med = {k: statistics.median(v) for k, v in times.items()}
            emit(workload=work, summary=True, runs=args.runs, nodes=next(iter(counters))[0], solutions=next(iter(counters))[1],
                 median_seconds={k: round(v, 5) for k, v in med.items()}, min_seconds={k: round(min(v), 5) for k, v in times.items()},
                 max_seconds={k: round(max(v), 5) for k, v in times.items()},
                 median_nodes_per_s={k: round(next(iter(counters))[0] / v, 1) for k, v in med.items()},
                 ratio_sink_ample_to_count=round(med["sink_ample"] / med["count"], 3), ratio_sink_4096_to_count=round(med["sink_4096"] / med["count"], 3),
                 ratio_small_to_sink_ample=round(med["small"] / med["sink_ample"], 3))
    out.close()
    ctx.close()


if __name__ == "__main__":
    main()
