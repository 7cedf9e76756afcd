"""The solution sink of the Interval forests (pcp_solution_sink_set), without a GPU: the header, the library and the bindings name it; the
refused combinations are ValueErrors before anything runs; SolutionSink.drain's bookkeeping on CPU tensors; the brute-force solution sets
test_forest_sink_gpu.py compares the device with are pinned as constants; and the schedule model has True nodes that are proper boxes —
the reason a solution is an (lb, ub) row and not a row of lower bounds."""
import inspect
import os
import re

import numpy as np
import pytest

import forest_sink_cases as K
from pcp_amd import search as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["lb", "ub", "tree", "count", "capacity", "reserved"]


def test_the_header_declares_and_the_library_exports_the_entry():
    """Fails without the feature: neither the header nor the ctypes and Rust lists name the entry."""
    import pcp_amd.engine as E
    import pcp_amd.search_forest as SF
    import test_abi
    with open(os.path.join(ROOT, "include", "pcp_hip.h")) as f:
        header = f.read()
    name = "pcp_solution_sink_set"
    assert re.search(r"\bint32_t\s+" + name + r"\s*\(\s*pcp_ctx\s*\*\s*\w+\s*,\s*const\s+pcp_solution_sink\s*\*", header)
    struct = re.search(r"typedef struct \{([^}]*)\} pcp_solution_sink;", header)
    assert struct and re.findall(r"(\w+);", struct.group(1)) == FIELDS
    assert "#define PCP_ABI_VERSION 8" in header
    assert name in E.ABI_SYMBOLS and hasattr(test_abi._built(), name)
    assert [f for f, _ in E.PcpSolutionSink._fields_] == FIELDS
    size, fields = test_abi._c_layout()["pcp_solution_sink"]
    import ctypes
    assert ctypes.sizeof(E.PcpSolutionSink) == size == 40
    assert [(f, getattr(E.PcpSolutionSink, f).offset) for f in FIELDS] == fields
    with open(os.path.join(ROOT, "integration", "pcp-hip-sys", "src", "lib.rs")) as f:
        rust = f.read()
    assert "pub fn " + name in rust and "pub struct pcp_solution_sink" in rust
    for fn in (E.Context.dfs_forest, SF.forest_search):
        p = inspect.signature(fn).parameters
        assert p["collect_solutions"].default is False and p["sink_capacity"].default == 4096
    assert hasattr(E.Context, "solution_sink_set") and E.SINK_FULL == 6


def test_refused_combinations_are_raised_before_anything_runs():
    import pcp_amd.engine as E
    from pcp_amd.search_forest import forest_bnb, forest_search
    dist = object()
    for kw in (dict(small=True, dist=dist), dict(formulas=True, dist=dist), dict(), dict(small=True, sink_capacity=0), dict(formulas=True, sink_capacity=-1),
               dict(small=True, brancher="enumerate", sink_capacity=0)):
        with pytest.raises(ValueError):
            E.Context.dfs_forest(None, None, None, collect_solutions=True, **kw)
        with pytest.raises(ValueError):
            forest_search(None, None, None, collect_solutions=True, **kw)
    with pytest.raises(ValueError):
        forest_search(None, None, None, collect_solutions=True, small=True, world=2)
    for kw in (dict(), dict(small=True), dict(small=True, brancher="enumerate")):
        with pytest.raises(ValueError):
            E.Context.dfs_forest_bnb(None, None, None, (0, "min"), collect_solutions=True, **kw)
        with pytest.raises(ValueError):
            forest_bnb(None, None, None, (0, "min"), collect_solutions=True, **kw)
    with pytest.raises(ValueError):
        E.SolutionSink(0, 3, "cpu")


def test_drain_bookkeeping_on_cpu_tensors():
    """Count below, at and above the capacity; the count is zeroed; rows are concatenated in order."""
    import torch
    import pcp_amd.engine as E
    cap, V = 3, 2
    sink = E.SolutionSink(cap, V, "cpu")
    assert sink.drain() == 0 and sink.rows()[0].shape == (0, V) and sink.rows()[2].shape == (0,)
    want_lb, want_ub, want_tree = [], [], []
    base = 0
    for drawn in (2, 3, 7, 0, 1):
        n = min(drawn, cap)
        sink.lb[:] = torch.arange(base, base + cap * V, dtype=torch.int32).reshape(cap, V)
        sink.ub[:] = sink.lb + 100
        sink.tree[:] = torch.arange(base, base + cap, dtype=torch.int32)
        sink.count[0] = drawn
        assert sink.drain() == n
        assert int(sink.count[0]) == 0
        want_lb += sink.lb[:n].tolist(); want_ub += sink.ub[:n].tolist(); want_tree += sink.tree[:n].tolist()
        base += 1000
        lb, ub, tree = sink.rows()
        assert lb.dtype == ub.dtype == tree.dtype == np.int32
        assert lb.tolist() == want_lb and ub.tolist() == want_ub and tree.tolist() == want_tree
    assert sink.overdrawn == 4 and sink.drains == 6
    sink.lb[:] = -1  # what was drained is the host's: the buffers can be written again
    assert sink.rows()[0].tolist() == want_lb
    s = sink.struct()
    assert (s.lb, s.ub, s.tree, s.count, s.capacity, s.reserved) == (sink.lb.data_ptr(), sink.ub.data_ptr(), sink.tree.data_ptr(), sink.count.data_ptr(), cap, 0)


@pytest.mark.parametrize("name", sorted(K.N_SOLUTIONS))
def test_the_brute_force_solution_sets(name):
    sols = K.brute(name)
    assert len(sols) == K.N_SOLUTIONS[name]
    V = len(K.root(name)[0])
    assert all(len(p) == V for p in sols)
    lb0, ub0 = K.root(name)
    assert all(all(l <= x <= u for x, l, u in zip(p, lb0, ub0)) for p in sols)


_SPLIT = {}


def split_boxes(name):
    """The host-stepped BinarySplit search over the oracle stand-in, once per model: (SearchStats, lb rows, ub rows of its True nodes)."""
    if name not in _SPLIT:
        k = K.KeepBoxes(K.stand_in(name))
        st = S.dfs(k, *K.root(name), all_solutions=True)
        _SPLIT[name] = (st, np.stack([b[0] for b in k.boxes]), np.stack([b[1] for b in k.boxes]))
    return _SPLIT[name]


@pytest.mark.parametrize("name", sorted(K.SPLIT_TREE))
def test_the_true_nodes_of_the_host_search_partition_the_solutions(name):
    st, lbs, ubs = split_boxes(name)
    proper = K.check_boxes(name, lbs, ubs)
    assert (st.num_nodes, st.num_solution, st.num_failed_node, proper) == K.SPLIT_TREE[name]
    assert K.multiset(lbs) == K.multiset(st.solutions)


def test_the_schedule_has_true_nodes_that_are_proper_boxes():
    """The pin: lower bounds alone lose solutions — 21 True nodes hold 24 schedules, three of them in boxes of two points."""
    st, lbs, ubs = split_boxes("sched3")
    wide = (lbs < ubs).any(axis=1)
    assert wide.sum() == 3 and st.num_solution == 21 < K.N_SOLUTIONS["sched3"] == 24
    assert sum(int(np.prod(u - l + 1)) for l, u in zip(lbs, ubs)) == 24
    assert all((lbs[i] < ubs[i]).sum() == 1 and (lbs[i] < ubs[i])[:3].any() for i in np.nonzero(wide)[0])  # one start variable, still free


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("name", ["queens6", "golomb4"])
def test_the_true_nodes_under_enumerate(name, val):
    rec = []
    st = S.dfs_enumerate(K.stand_in(name), *K.root(name), all_solutions=True, val=val, record=rec)
    true = [r for r in rec if r[3] == 1]
    assert K.check_boxes(name, [r[4] for r in true], [r[5] for r in true]) == 0 and st.num_solution == K.N_SOLUTIONS[name]
