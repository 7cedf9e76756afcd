"""The search drivers, pinned call for call on the CPU: pcp_amd.search_device.DeviceSearch over the oracle-backed stand-in contexts, and the host
loops search.dfs / search.dfs_set, against traces recorded BEFORE the drivers were folded into one loop and one round
(tests/golden/search_traces.json).

A trace of DeviceSearch is every call it makes on its context — the method, its scalar arguments, and for every tensor argument which of
DeviceSearch's buffers it views and at which row — followed by the final DeviceSearchStats.  Arguments are bound to the signatures of
pcp_amd.engine.Context, so an optional argument left out and the same argument passed as its default are one trace.  A trace of a host loop is
its calls on the context (arrays as shape + CRC) and the complete SearchStats.

The module uses public API only, so it runs unmodified on the commit before a change to the drivers.  The golden file is recorded THERE (a
checkout of that commit with this file copied in), never from the changed code:

    python tests/test_search_trace_cpu.py > tests/golden/search_traces.json

search.dfs_enumerate is not here: it builds CUDA tensors itself and no stand-in runs it without a GPU; tests/test_branch_excl.py and
tests/test_neq_excl.py drive it on the device."""
import dataclasses
import inspect
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

import torch  # noqa: E402

import pcp_amd.engine as E  # noqa: E402
from pcp_amd import model as M  # noqa: E402
from pcp_amd import search as S  # noqa: E402
from pcp_amd.search_device import DeviceSearch  # noqa: E402

from oracle_ctx import OracleCtx, OracleDeviceCtx  # noqa: E402
from test_bnb_host import OracleBnbDeviceCtx, OracleSetCtx, _golomb, _kat_model  # noqa: E402
from test_enum_search_cpu import EnumOracleCtx  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "search_traces.json")
# DeviceSearch's buffers, in the order they are matched: `counts`, `best` and `improved` before `round_buf`, whose views they may be
BUFFERS = ("lb", "ub", "act", "bits", "dirty", "status", "counts", "best", "improved", "best_lb", "best_ub", "best_bits", "ex", "eoff", "round_buf")


SMALL = (32, 20)  # rows and arena entries of the small Enumerate run: 6-queens then merges, compacts and takes fewer nodes (checked from the golden file)


def _jsonable(x):
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    if isinstance(x, dict):
        return {str(k): _jsonable(v) for k, v in x.items()}
    return x


def _stats(st):
    return _jsonable(dataclasses.asdict(st))


class DeviceRecorder:
    """A context that passes everything on to `ctx` and logs every method call made on it."""

    def __init__(self, ctx):
        self._ctx, self.log, self.ds = ctx, [], None

    def __getattr__(self, name):
        a = getattr(self._ctx, name)
        if not callable(a):
            return a

        def call(*args, **kw):
            bound = inspect.signature(getattr(E.Context, name)).bind(None, *args, **kw)
            bound.apply_defaults()
            self.log.append([name] + [self._describe(v) for k, v in list(bound.arguments.items())[1:]])
            return a(*args, **kw)
        return call

    def _describe(self, v):
        if v is None or isinstance(v, (bool, int, str)):
            return v
        if isinstance(v, dict):
            return {k: self._describe(v[k]) for k in sorted(v)}
        if isinstance(v, torch.Tensor):
            for name in BUFFERS:
                b = getattr(self.ds, name, None)
                if isinstance(b, torch.Tensor):
                    off = v.data_ptr() - b.data_ptr()
                    if 0 <= off < b.numel() * b.element_size():
                        return f"{name}@{off // (b.stride(0) * b.element_size())}"
        return None


def _device_trace(ctx, lb0, ub0, ds_kw, run_kw):
    rec = DeviceRecorder(ctx)
    ds = DeviceSearch(rec, device=torch.device("cpu"), **ds_kw)
    rec.ds = ds
    st = ds.run(lb0, ub0, **run_kw)
    out = {"calls": rec.log, "stats": _stats(st)}
    if ds.brancher == "enumerate":
        out["arena_events"] = dict(ds.arena_events)
    return out


def _queens(n):
    return n, M.nqueens_props(n), np.ones(n, np.int32), np.full(n, n, np.int32)


def _device_cases():
    """name -> a function that runs the case and returns its trace."""
    n, props, lb0, ub0 = _queens(6)
    cases = {}

    def add(name, make_ctx, root, ds_kw, run_kw):
        cases[name] = lambda: _device_trace(make_ctx(), *root, ds_kw, run_kw)

    plain = lambda: OracleDeviceCtx(n, props)
    every = dict(all_solutions=True, keep_solutions=1 << 20)
    for batch in (1, 4, 7):
        add(f"split/implicit/batch{batch}", plain, (lb0, ub0), dict(batch=batch, implicit=True), every)
    add("split/implicit/batch7/capacity24", plain, (lb0, ub0), dict(batch=7, capacity=24, implicit=True), every)
    add("split/implicit/nohints/batch4", plain, (lb0, ub0), dict(batch=4, implicit=True, hints=False), every)
    add("split/explicit/batch4", plain, (lb0, ub0), dict(batch=4, implicit=False), every)
    add("split/cells/batch5", plain, (lb0, ub0), dict(batch=5, implicit=True, cells=True), every)
    # stopped early: the limit falls inside a batch of 7 (on an inner node, a failure, a solution), or the first solution ends the search
    for limit in (10, 17, 24, 30, 31):
        for all_solutions in (False, True):
            add(f"split/implicit/batch7/limit{limit}/all{int(all_solutions)}", plain, (lb0, ub0), dict(batch=7, implicit=True),
                dict(all_solutions=all_solutions, node_limit=limit, keep_solutions=2))
    add("split/cells/batch7/limit31", plain, (lb0, ub0), dict(batch=7, implicit=True, cells=True), dict(all_solutions=True, node_limit=31, keep_solutions=2))
    add("split/implicit/batch7/first", plain, (lb0, ub0), dict(batch=7, implicit=True), dict(all_solutions=False, keep_solutions=2))
    enum = lambda: EnumOracleCtx(n, props)
    for val in ("middle", "min"):
        for batch in (1, 3):
            add(f"enumerate/{val}/batch{batch}", enum, (lb0, ub0), dict(batch=batch, implicit=True, brancher="enumerate", val=val), every)
        add(f"enumerate/{val}/batch3/limit20", enum, (lb0, ub0), dict(batch=3, implicit=True, brancher="enumerate", val=val),
            dict(all_solutions=True, node_limit=20, keep_solutions=2))
        add(f"enumerate/{val}/batch7/small", enum, (lb0, ub0), dict(batch=7, capacity=SMALL[0], excl_capacity=SMALL[1], implicit=True, brancher="enumerate", val=val), every)
    V, kprops, klb, kub, var = _kat_model()
    for mode in ("min", "max"):
        for batch in (1, 4):
            for implicit in (True, False):
                add(f"bnb/{mode}/batch{batch}/{'implicit' if implicit else 'explicit'}", lambda: OracleBnbDeviceCtx(V, kprops), (klb, kub),
                    dict(batch=batch, capacity=256, implicit=implicit, objective=(var, mode)), {})
    return cases


class HostRecorder:
    """The same for the host loops: arrays are logged as shape + CRC of their bytes."""

    def __init__(self, ctx):
        self._ctx, self.log = ctx, []

    def __getattr__(self, name):
        a = getattr(self._ctx, name)
        if not callable(a):
            return a

        def call(*args, **kw):
            self.log.append([name] + [self._describe(v) for v in args] + [[k, self._describe(kw[k])] for k in sorted(kw)])
            return a(*args, **kw)
        return call

    @staticmethod
    def _describe(v):
        if isinstance(v, np.ndarray):
            return [list(v.shape), str(v.dtype), zlib.crc32(np.ascontiguousarray(v).tobytes())]
        return v if v is None or isinstance(v, (bool, int, str)) else None


def _host_cases():
    n, props, lb0, ub0 = _queens(6)
    cases = {}

    def add(name, make_ctx, fn, args, kw):
        def run():
            rec = HostRecorder(make_ctx())
            return {"calls": rec.log, "stats": _stats(fn(rec, *args, **kw))}
        cases[name] = run

    V, kprops, klb, kub, kvar = _kat_model()
    GV, gprops, glb, gub, gvar = _golomb(5, 20)
    for batch in (1, 3, 8):
        for limit in (0, 23):
            for all_solutions in (False, True):
                tag = f"batch{batch}/limit{limit}/all{int(all_solutions)}"
                kw = dict(batch=batch, node_limit=limit, all_solutions=all_solutions)
                add(f"dfs/{tag}", lambda: OracleCtx(n, props), S.dfs, (lb0, ub0), kw)
                for implicit in (True, False):
                    add(f"dfs_set/{'implicit' if implicit else 'explicit'}/{tag}", lambda: OracleSetCtx(n, props, 1, 1), S.dfs_set, (lb0, ub0, 1), dict(kw, implicit=implicit))
            for mode in ("min", "max"):
                tag = f"batch{batch}/limit{limit}/{mode}"
                kw = dict(batch=batch, node_limit=limit and 7, objective=(kvar, mode))
                add(f"dfs/kat/{tag}", lambda: OracleCtx(V, kprops), S.dfs, (klb, kub), kw)
                add(f"dfs_set/kat/{tag}", lambda: OracleSetCtx(V, kprops, 1, 0), S.dfs_set, (klb, kub, 0), kw)
                add(f"dfs_set/kat/explicit/{tag}", lambda: OracleSetCtx(V, kprops, 1, 0), S.dfs_set, (klb, kub, 0), dict(kw, implicit=False))
                add(f"dfs/golomb5/{tag}", lambda: OracleCtx(GV, gprops), S.dfs, (glb, gub), dict(kw, node_limit=limit))
    return cases


DEVICE_CASES = _device_cases()
HOST_CASES = _host_cases()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def _compare(got, want):
    got = json.loads(json.dumps(got))
    assert got["stats"] == want["stats"]
    assert got.get("arena_events") == want.get("arena_events")
    assert len(got["calls"]) == len(want["calls"])
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"call {i}"


@pytest.mark.parametrize("name", sorted(DEVICE_CASES))
def test_device_search_trace(name, golden):
    _compare(DEVICE_CASES[name](), golden["device"][name])


@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_host_loop_trace(name, golden):
    _compare(HOST_CASES[name](), golden["host"][name])


def test_the_golden_traces_cover_what_they_are_for(golden):
    """The recorded runs took the paths they were chosen for: the small buffers merged, compacted and narrowed rounds; the small row buffer
    compacted and took fewer nodes per round (more rounds over the same tree); nothing else is in the file."""
    dev, host = golden["device"], golden["host"]
    assert sorted(dev) == sorted(DEVICE_CASES) and sorted(host) == sorted(HOST_CASES)
    ev = dev["enumerate/middle/batch7/small"]["arena_events"]
    assert ev["merge"] >= 1 and ev["compact"] >= 1 and ev["fewer"] >= 1, ev
    ev = dev["enumerate/min/batch7/small"]["arena_events"]
    assert ev["merge"] >= 1 and ev["compact"] >= 1 and ev["fewer"] == 0, ev  # (MinVal's value is a bound: no list is ever written)
    full, tight = dev["split/implicit/batch7"], dev["split/implicit/batch7/capacity24"]
    assert tight["stats"]["rounds"] > full["stats"]["rounds"] and tight["stats"]["num_nodes"] == full["stats"]["num_nodes"]
    for name, t in dev.items():
        assert 2 <= len(t["calls"]) < 1200, name
    assert any(t["stats"]["best"] is not None for k, t in dev.items() if k.startswith("bnb/"))
    assert dev["split/implicit/batch7/limit31/all1"]["stats"]["num_nodes"] == 31


if __name__ == "__main__":
    out = {"device": {k: DEVICE_CASES[k]() for k in sorted(DEVICE_CASES)}, "host": {k: HOST_CASES[k]() for k in sorted(HOST_CASES)}}
    json.dump(out, sys.stdout, separators=(",", ":"), sort_keys=True)
    sys.stdout.write("\n")
