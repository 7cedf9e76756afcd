"""The host drivers of the Interval search forests, pinned call for call on the device: Context.dfs_forest / dfs_forest_bnb / dfs_forest_enum /
dfs_forest_neq_solutions and search_forest.forest_search / forest_bnb / forest_enumerate / forest_solutions, against traces recorded BEFORE
the drivers were folded into one private runner (tests/golden/forest_traces.json).

A trace is every call the driver makes on the library whose name starts with ``pcp_dfs_forest`` or is ``pcp_solution_sink_set`` — the entry's
name, every scalar argument, for every pointer argument whether it is null, and of the structs passed by reference their scalar fields (the
state's ``capacity``, the exclusions' ``path_capacity`` and ``val``, a sink's ``capacity``, an objective's ``var`` and ``mode``) and which of
their pointers are null; no address is recorded — followed by the result dict and what the driver left in ``info``: arrays as shape + CRC,
the collected solutions sorted before they are hashed.

Two classes of cases.  EXACT: no objective, and a sink (if any) that never fills — every tree does the same from run to run and under either
steal, so the whole log is compared call for call and the whole result, ``per_tree`` included.  TIMING: branch and bound (the trees of one
launch share the incumbent while they run) and a sink of two rows that fills (which tree draws the ticket beyond the capacity is an order in
time) — there the log is compared with runs of identical consecutive calls collapsed to one, and of the result what is pinned elsewhere:
the set of solution boxes, the optimum, and the objective's value in ``best_solution``.  Those cases run under steal="host" only, with
stacks and paths that need not grow, so that their collapsed log does not depend on the timing either.

The module uses public API only, so it runs unmodified on the commit before a change to the drivers.  The golden file is recorded THERE, on
the GPU (a checkout of that commit with this file copied in), never from the changed code — twice, and a case whose two recordings differ
does not belong in the exact class:

    python tests/test_forest_trace_gpu.py > tests/golden/forest_traces.json
"""
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):  # (run as a script: the repository root and tests/ are not on the path yet)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import form_forest_cases as FC  # noqa: E402
import forest_sink_cases as K  # noqa: E402
import small_forest_cases as SC  # noqa: E402
from pcp_amd import model as M  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "forest_traces.json")
STEALS = ("host", "device")


# ------------------------------------------------------------------------------------------------ the recorder
def _struct(s):
    """The scalar fields of a ctypes struct, and which of its pointer fields are null."""
    out = {}
    for name, typ in s._fields_:
        if name == "reserved":
            continue
        v = getattr(s, name)
        out[name] = ("ptr" if v else None) if typ is C.c_void_p else int(v)
    return out


def _arg(a):
    if a is None or isinstance(a, (bool, int)):
        return None if a is None else int(a)
    if isinstance(a, C.c_void_p):
        return "ptr" if a.value else None
    if isinstance(a, C.Structure):
        return _struct(a)
    if hasattr(a, "_obj"):  # ctypes.byref(struct)
        return _struct(a._obj)
    if hasattr(a, "contents"):  # ctypes.pointer(struct)
        return _struct(a.contents) if a else None
    if hasattr(a, "value"):
        return int(a.value)
    raise TypeError(f"an argument the recorder does not know: {a!r}")


class LibRecorder:
    """Stands in for Context._L: passes every attribute on, and logs the calls of the forest entries."""

    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not (name.startswith("pcp_dfs_forest") or name == "pcp_solution_sink_set"):
            return f

        def call(*args):
            self.log.append([name] + [_arg(a) for a in args[1:]])  # (args[0]: the context's handle)
            return f(*args)
        return call


def _crc(a):
    a = np.ascontiguousarray(a)
    return [list(a.shape), str(a.dtype), zlib.crc32(a.tobytes())]


def _describe(v):
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, np.integer):
        return int(v)
    if isinstance(v, float):
        return None  # (wall times)
    if isinstance(v, np.ndarray):
        return _crc(v)
    if hasattr(v, "detach"):  # a torch tensor
        return _crc(v.detach().cpu().numpy())
    if isinstance(v, dict):
        return {str(k): _describe(v[k]) for k in sorted(v)}
    if isinstance(v, (list, tuple)):
        return [_describe(x) for x in v]
    raise TypeError(f"a value the recorder does not know: {v!r}")


def _sorted_rows(*cols):
    rows = np.concatenate([np.asarray(c, np.int64).reshape(len(cols[0]), -1) for c in cols], axis=1)
    return _crc(rows[np.lexsort(rows.T[::-1])] if len(rows) else rows)


def _result(r, objective=None):
    r = dict(r)
    out = {}
    if "solutions_lb" in r:
        lb, ub, tree = r.pop("solutions_lb"), r.pop("solutions_ub"), r.pop("solution_tree")
        out["boxes"] = _sorted_rows(lb, ub)            # the SET of solutions
        out["boxes_by_tree"] = _sorted_rows(lb, ub, tree)  # ... and which tree wrote each
    if objective is not None:
        row = r.get("best_solution")
        out["best_value"] = None if row is None else int(row[objective[0]])
    out["result"] = _describe(r)
    return out


def trace(ctx, run, objective=None):
    """run(info) on ``ctx`` with the library recorded: {"calls", "result", "info", ...}."""
    lib = ctx._L
    rec = LibRecorder(lib)
    ctx._L = rec
    info = {}
    try:
        r = run(info)
    finally:
        ctx._L = lib
    return dict(_result(r, objective), calls=rec.log, info=_describe(info))


# ------------------------------------------------------------------------------------------------ the models
def _push(ctx, vs, cs):
    M.push_model(ctx, cs, len(vs))
    lb0, ub0 = vs.bounds()
    return np.ascontiguousarray(lb0, np.int32), np.ascontiguousarray(ub0, np.int32)


def queens6(ctx):
    ctx.set_model(6, M.nqueens_props(6))
    return np.ones(6, np.int32), np.full(6, 6, np.int32), None


def golomb5(ctx):
    vs, cs, var = SC.golomb(5)
    return _push(ctx, vs, cs) + (var,)


def sched3(ctx):
    return _push(ctx, *K.build("sched3")) + (None,)


def c4mk(ctx):
    vs, cs, mk = FC.schedule("C4mk")
    return _push(ctx, vs, cs) + (mk,)


MODELS = {"queens6": (queens6, 6), "golomb5": (golomb5, 8), "sched3": (sched3, 6), "c4mk": (c4mk, 6)}  # name -> (push, trees)


def _roots(ctx, model, val=None, objective=None):
    """Push the model; the open nodes of its breadth-first expansion: (lb rows, ub rows, lists or None, lb0, ub0, objective variable)."""
    from pcp_amd.search_forest import seed_roots_interval
    push, trees = MODELS[model]
    lb0, ub0, var = push(ctx)
    if val is None:
        rl, ru, _ = seed_roots_interval(ctx, lb0, ub0, trees)
        return rl, ru, None, lb0, ub0, var
    rl, ru, _, lists = seed_roots_interval(ctx, lb0, ub0, trees, brancher="enumerate", val=val)
    return rl, ru, lists, lb0, ub0, var


# ------------------------------------------------------------------------------------------------ the cases
TIGHT = dict(steps_per_launch=4, capacity=2, max_capacity=256)   # two-row stacks: they grow (error 1); short launches: trees finish apart and steal
ROOMY = dict(steps_per_launch=8, capacity=64)                    # nothing grows


def _cases():
    """name -> (class, run(ctx, steal) -> trace).  An EXACT case runs under both steals, a TIMING case under steal="host"."""
    cases = {}

    def add(name, model, call, val=None, timing=False, objective=False):
        def run(ctx, steal):
            rl, ru, lists, lb0, ub0, var = _roots(ctx, model, val=val)
            env = dict(ctx=ctx, rl=rl, ru=ru, lists=lists, lb0=lb0, ub0=ub0, var=var, steal=steal)
            return trace(ctx, lambda info: call(env, info), objective=(var, "min") if objective else None)
        cases[name] = ("timing" if timing else "exact", run)

    ctx_call = lambda method, *a, **kw: (lambda e, info: getattr(e["ctx"], method)(e["rl"], e["ru"], *[x(e) for x in a], steal=e["steal"], info=info,
                                                                                  **{k: (v(e) if callable(v) else v) for k, v in kw.items()}))
    lists = lambda e: e["lists"]
    obj = lambda e: (e["var"], "min")

    # --- N-queens 6, the all-XNeqY in-kernel forest
    add("queens6/plain", "queens6", ctx_call("dfs_forest", **TIGHT))
    add("queens6/plain/no_hints/stop", "queens6", ctx_call("dfs_forest", hints=False, stop_on_solution=True, want_solution=True, **ROOMY))
    add("queens6/plain/node_limit", "queens6", ctx_call("dfs_forest", node_limit_per_tree=5, **ROOMY))
    add("queens6/plain/node_budget", "queens6", ctx_call("dfs_forest", node_budget=20, **TIGHT))
    add("queens6/plain/no_rebalance", "queens6", ctx_call("dfs_forest", rebalance=False, **ROOMY))
    add("queens6/enum/middle", "queens6", ctx_call("dfs_forest_enum", val="middle", root_excl=lists, forest="neq", path_capacity=1, **TIGHT), val="middle")
    add("queens6/enum/min", "queens6", ctx_call("dfs_forest_enum", val="min", root_excl=lists, forest="neq", path_capacity=0, **TIGHT), val="min")
    add("queens6/enum/middle/no_hints", "queens6", ctx_call("dfs_forest_enum", val="middle", root_excl=lists, forest="neq", hints=False, **ROOMY), val="middle")
    add("queens6/sink/split", "queens6", ctx_call("dfs_forest_neq_solutions", sink_capacity=64, **TIGHT))
    add("queens6/sink/enum/middle", "queens6", ctx_call("dfs_forest_neq_solutions", brancher="enumerate", val="middle", root_excl=lists, sink_capacity=64,
                                                         path_capacity=1, **TIGHT), val="middle")
    add("queens6/sink/enum/min", "queens6", ctx_call("dfs_forest_neq_solutions", brancher="enumerate", val="min", root_excl=lists, sink_capacity=64, **ROOMY), val="min")
    add("queens6/sink/fills", "queens6", ctx_call("dfs_forest_neq_solutions", sink_capacity=2, **ROOMY), timing=True)

    # --- a Golomb ruler of five marks, the small-store forest
    add("golomb5/plain", "golomb5", ctx_call("dfs_forest", small=True, **TIGHT))
    add("golomb5/plain/stop", "golomb5", ctx_call("dfs_forest", small=True, stop_on_solution=True, want_solution=True, **ROOMY))
    add("golomb5/plain/node_limit", "golomb5", ctx_call("dfs_forest", small=True, node_limit_per_tree=7, **ROOMY))
    add("golomb5/enum/middle", "golomb5", ctx_call("dfs_forest", small=True, brancher="enumerate", val="middle", root_excl=lists, path_capacity=1, **TIGHT), val="middle")
    add("golomb5/enum/min", "golomb5", ctx_call("dfs_forest_enum", val="min", root_excl=lists, path_capacity=0, **TIGHT), val="min")
    add("golomb5/collect", "golomb5", ctx_call("dfs_forest", small=True, collect_solutions=True, sink_capacity=4096, **TIGHT))
    add("golomb5/enum/collect", "golomb5", ctx_call("dfs_forest_enum", val="middle", root_excl=lists, collect_solutions=True, sink_capacity=4096, **ROOMY), val="middle")
    add("golomb5/collect/fills", "golomb5", ctx_call("dfs_forest", small=True, collect_solutions=True, sink_capacity=2, **ROOMY), timing=True)
    add("golomb5/bnb", "golomb5", ctx_call("dfs_forest_bnb", obj, small=True, **ROOMY), timing=True, objective=True)
    add("golomb5/bnb/enum", "golomb5", ctx_call("dfs_forest_bnb", obj, small=True, brancher="enumerate", val="middle", root_excl=lists, **ROOMY),
        val="middle", timing=True, objective=True)

    # --- schedules, the formula-store forest (the three-task one; with a makespan to minimise, the four-task one)
    add("sched3/plain", "sched3", ctx_call("dfs_forest", formulas=True, **TIGHT))
    add("sched3/plain/node_budget", "sched3", ctx_call("dfs_forest", formulas=True, node_budget=30, **ROOMY))
    add("sched3/enum/middle", "sched3", ctx_call("dfs_forest_enum", val="middle", root_excl=lists, path_capacity=1, **TIGHT), val="middle")
    add("sched3/enum/min", "sched3", ctx_call("dfs_forest_enum", val="min", root_excl=lists, **ROOMY), val="min")
    add("sched3/collect", "sched3", ctx_call("dfs_forest", formulas=True, collect_solutions=True, sink_capacity=4096, **TIGHT))
    add("sched3/enum/collect", "sched3", ctx_call("dfs_forest_enum", val="middle", root_excl=lists, collect_solutions=True, sink_capacity=4096, **ROOMY), val="middle")
    add("sched3/collect/fills", "sched3", ctx_call("dfs_forest", formulas=True, collect_solutions=True, sink_capacity=2, **ROOMY), timing=True)
    add("c4mk/bnb", "c4mk", ctx_call("dfs_forest_bnb", obj, **ROOMY), timing=True, objective=True)
    add("c4mk/enum/bnb", "c4mk", ctx_call("dfs_forest_enum", val="middle", objective=obj, root_excl=lists, **ROOMY), val="middle", timing=True, objective=True)

    # --- the drivers above the context, once each and on every forest they choose between
    def driver(fn, *a, **kw):
        def call(e, info):
            import pcp_amd.search_forest as F
            return getattr(F, fn)(e["ctx"], e["lb0"], e["ub0"], *[x(e) for x in a], steal=e["steal"], info=info,
                                  **{k: (v(e) if callable(v) else v) for k, v in kw.items()})
        return call

    small = dict(n_trees=8, steps_per_launch=4, capacity=2)
    add("drivers/forest_search/queens6", "queens6", driver("forest_search", n_trees=6, steps_per_launch=4, capacity=2))
    add("drivers/forest_search/queens6/node_limit", "queens6", driver("forest_search", n_trees=6, steps_per_launch=4, node_limit=40))
    add("drivers/forest_search/golomb5/collect", "golomb5", driver("forest_search", small=True, collect_solutions=True, **small))
    add("drivers/forest_search/sched3/enum", "sched3", driver("forest_enumerate", val="min", collect_solutions=True, n_trees=6, steps_per_launch=4, capacity=2))
    add("drivers/forest_enumerate/golomb5", "golomb5", driver("forest_enumerate", val="middle", path_capacity=1, **small))
    add("drivers/forest_enumerate/queens6/neq", "queens6", driver("forest_enumerate", val="middle", forest="neq", n_trees=6, steps_per_launch=4, capacity=2))
    add("drivers/forest_solutions/queens6/neq", "queens6", driver("forest_solutions", forest="neq", n_trees=6, steps_per_launch=4, capacity=2))
    add("drivers/forest_solutions/queens6/neq/enum", "queens6", driver("forest_solutions", forest="neq", brancher="enumerate", val="min", n_trees=6, steps_per_launch=4, capacity=2))
    add("drivers/forest_solutions/golomb5", "golomb5", driver("forest_solutions", **small))
    add("drivers/forest_solutions/sched3/enum", "sched3", driver("forest_solutions", brancher="enumerate", val="middle", n_trees=6, steps_per_launch=4, capacity=2))
    add("drivers/forest_bnb/c4mk", "c4mk", driver("forest_bnb", obj, n_trees=6, steps_per_launch=8), timing=True, objective=True)
    add("drivers/forest_bnb/golomb5", "golomb5", driver("forest_bnb", obj, small=True, n_trees=8, steps_per_launch=8), timing=True, objective=True)
    add("drivers/forest_enumerate/c4mk/objective", "c4mk", driver("forest_enumerate", objective=obj, n_trees=6, steps_per_launch=8), timing=True, objective=True)
    return cases


CASES = _cases()
RUNS = sorted((name, steal) for name, (cls, _) in CASES.items() for steal in (STEALS if cls == "exact" else STEALS[:1]))


def run_case(ctx, name, steal):
    return CASES[name][1](ctx, steal)


def pack(traces):
    """The golden file: every distinct call once, in a table, and each trace's log as indices into it (a log is hundreds of launches that
    differ in a word or two)."""
    table, index = [], {}
    for t in traces.values():
        keys = [json.dumps(c, sort_keys=True) for c in t["calls"]]
        for k, c in zip(keys, t["calls"]):
            if k not in index:
                index[k] = len(table)
                table.append(c)
        t["calls"] = [index[k] for k in keys]
    return {"table": table, "traces": traces}


def unpack(packed):
    return {name: dict(t, calls=[packed["table"][i] for i in t["calls"]]) for name, t in packed["traces"].items()}


def collapsed(calls):
    """The log with runs of identical consecutive calls collapsed to one."""
    out = []
    for c in calls:
        if not out or out[-1] != c:
            out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return unpack(json.load(open(GOLDEN)))


@pytest.mark.parametrize("name,steal", RUNS)
def test_forest_driver_trace(ctx, golden, name, steal):
    got = json.loads(json.dumps(run_case(ctx, name, steal)))
    want = golden[f"{name}@{steal}"]
    if CASES[name][0] == "exact":
        assert got["result"] == want["result"]
        assert got.get("boxes_by_tree") == want.get("boxes_by_tree")
        assert got["info"] == want["info"]
        assert len(got["calls"]) == len(want["calls"])
        for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
            assert g == w, f"call {i}"
    else:
        assert collapsed(got["calls"]) == collapsed(want["calls"])
        assert got.get("boxes") == want.get("boxes")
        assert got["result"].get("best") == want["result"].get("best") and got.get("best_value") == want.get("best_value")
        assert got["result"]["error"] == 0 and got["result"].get("open", 0) == 0


def test_three_quarters_of_the_runs_are_compared_exactly():
    exact = sum(1 for name, _ in RUNS if CASES[name][0] == "exact")
    assert 4 * exact >= 3 * len(RUNS), (exact, len(RUNS))


def test_the_golden_traces_cover_what_they_are_for(golden):
    """The recorded runs took the paths they were chosen for: every entry point of the Interval forests was called, stacks and paths grew,
    trees stole under both steals, a full sink was drained, the limits ended searches early; nothing else is in the file."""
    assert sorted(golden) == sorted(f"{n}@{s}" for n, s in RUNS)
    called = {c[0] for t in golden.values() for c in t["calls"]}
    assert called >= {"pcp_dfs_forest_device", "pcp_dfs_forest_device_form", "pcp_dfs_forest_device_small", "pcp_dfs_forest_device_form_bnb",
                      "pcp_dfs_forest_device_small_bnb", "pcp_dfs_forest_device_small_enum", "pcp_dfs_forest_device_form_enum", "pcp_dfs_forest_device_neq_enum",
                      "pcp_dfs_forest_device_neq_sink", "pcp_dfs_forest_steal", "pcp_solution_sink_set"}, called
    info = lambda name, steal="host": golden[f"{name}@{steal}"]["info"]
    for steal in STEALS:
        for name in ("queens6/plain", "queens6/enum/middle", "golomb5/plain", "golomb5/enum/middle", "sched3/plain", "sched3/enum/middle"):
            assert info(name, steal)["grown"] >= 1 and info(name, steal)["steals"] >= 1, (name, steal, info(name, steal))
        for name in ("queens6/enum/middle", "golomb5/enum/middle", "sched3/enum/middle"):
            assert info(name, steal)["first_steal"] is not None, (name, steal)
        for name in ("queens6/enum/middle", "golomb5/enum/middle"):  # (the schedule's roots arrive with lists longer than any path it then needs)
            assert info(name, steal)["path_grown"] >= 1, (name, steal)
        assert info("queens6/sink/split", steal)["drains"] == 0 and info("golomb5/collect", steal)["drains"] == 0 and info("sched3/collect", steal)["drains"] == 0
    for name in ("queens6/sink/fills", "golomb5/collect/fills", "sched3/collect/fills"):
        assert info(name)["drains"] >= 1, name
    res = lambda name: golden[f"{name}@host"]["result"]
    assert res("queens6/plain/no_hints/stop")["solutions"] >= 1 and res("queens6/plain/no_hints/stop")["open"] > 0
    assert res("queens6/plain/node_limit")["open"] > 0 and res("queens6/plain/node_budget")["open"] > 0
    assert 20 <= res("queens6/plain/node_budget")["nodes"] < res("queens6/plain")["nodes"]
    assert res("golomb5/bnb")["best"] == res("golomb5/bnb/enum")["best"] == SC.OPTIMUM[5]
    # Enumerate under dfs_forest_bnb goes to the Enumerate entry with the objective, never to the bnb entry
    names = {c[0] for c in golden["golomb5/bnb/enum@host"]["calls"]}
    assert names == {"pcp_dfs_forest_device_small_enum"} and all(c[4] is not None for c in golden["golomb5/bnb/enum@host"]["calls"]), names


if __name__ == "__main__":
    import pcp_amd.engine as E
    c = E.Context(0)
    out = {}
    for name, steal in RUNS:
        out[f"{name}@{steal}"] = t = run_case(c, name, steal)
        i, r = t["info"], t["result"]
        print(f"{name}@{steal}: calls {len(t['calls'])} launches {r.get('launches')} nodes {r.get('nodes')} solutions {r.get('solutions')} steals {i.get('steals')} "
              f"grown {i.get('grown')} path_grown {i.get('path_grown')} drains {i.get('drains')} best {r.get('best')}", file=sys.stderr)
    c.close()
    json.dump(pack(json.loads(json.dumps(out))), sys.stdout, separators=(",", ":"), sort_keys=True)
    sys.stdout.write("\n")
