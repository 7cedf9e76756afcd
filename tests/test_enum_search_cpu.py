"""Enumerate on the device, the parts that need no GPU: the ABI list, and DeviceSearch(brancher="enumerate") — the open-node stack with its
exclusion arena — driven on CPU tensors by an oracle-backed stand-in context.  The stand-in's propagate_device_excl is the oracle with the
node's XNeqY(x, Constant(v)) units allocated behind the model's (Branch::distribute, branch.rs:36-55); its branch_device_excl is
pcp_amd.search.branch_enumerate plus the counts of pcp_branch_device_excl.  The judge is a plain loop in this file: one node at a time from a
Python list, oracle consistency, branch_enumerate."""
import json
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from pcp_amd import model as M
from pcp_amd import search as S
import pcp_amd.engine as E
from pcp_amd.search_device import DeviceSearch

from oracle_ctx import OracleDeviceCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_lists_the_entry():
    assert "pcp_branch_device_excl" in E.ABI_SYMBOLS  # (tests/test_abi.py then checks the header and the export)
    header = open(os.path.join(ROOT, "include", "pcp_hip.h")).read()
    assert re.search(r"#define\s+PCP_VAL_MIDDLE\s+0u", header) and re.search(r"#define\s+PCP_VAL_MIN\s+1u", header)
    assert "pcp_branch_device_excl" in open(os.path.join(ROOT, "integration", "pcp-hip-sys", "src", "lib.rs")).read()
    assert (E.VAL_MODES["middle"], E.VAL_MODES["min"]) == (0, 1)


def _with_units(props, ex):
    """The model's propagators and, behind them, x != Constant(v) for every entry of a node's list."""
    if not len(ex):
        return props
    p = np.zeros(len(ex), dtype=M.PROP_DTYPE)
    p["kind"] = M.NEQ
    p["var"][:] = [0, M.PCP_CONST, M.PCP_NOVAR]
    p["var"][:, 0] = [int(e[0]) for e in ex]
    p["off"][:, 1] = [int(e[1]) for e in ex]
    p["group"] = np.arange(len(p)) + int(props["group"].max()) + 1
    return np.concatenate([props, p])


_FIXPOINTS = {}  # (n, lb, ub, exclusions) -> (status, lb, ub): computed once, shared by every test and never changed


def _consistency(n, props, lb, ub, ex):
    key = (n, lb.tobytes(), ub.tobytes(), np.ascontiguousarray(ex, np.int32).tobytes())
    if key not in _FIXPOINTS:
        r = orc.OracleModel(n, _with_units(props, ex)).consistency(lb.reshape(1, -1), ub.reshape(1, -1), None)
        _FIXPOINTS[key] = (int(r[3][0]), r[0][0].copy(), r[1][0].copy())
    return _FIXPOINTS[key]


class EnumOracleCtx(OracleDeviceCtx):
    """OracleDeviceCtx plus the two entry points of the Enumerate round."""

    def __init__(self, n_vars, props):
        super().__init__(n_vars, props)
        self._props = props
        self.branch_calls = 0

    def propagate_device_excl(self, n, lb_in, ub_in, lb_out, ub_out, active_out, status, excl_off, excl, stream=0, dirty=None):
        import torch
        assert active_out is None
        L, U = lb_in[:n].numpy().copy(), ub_in[:n].numpy().copy()
        off, ex = excl_off[:n + 1].numpy(), excl.numpy()
        if dirty is not None:
            d = dirty[:n].numpy()
            assert ((d == -1) | ((d >= 0) & (d < self.n_vars))).all(), d
            self.hints_seen += int((d >= 0).sum())
        for i in range(n):
            assert (L[i] <= U[i]).all()  # (an Enumerate child is never empty)
            st, lb, ub = _consistency(self.n_vars, self._props, L[i], U[i], ex[off[i]:off[i + 1]])
            status[i] = st
            lb_out[i] = torch.from_numpy(lb)
            ub_out[i] = torch.from_numpy(ub)
        self._stats["nodes"] += n

    def branch_device_excl(self, n, lb, ub, status, excl_off, excl, val, child_lb, child_ub, child_excl_off, child_excl, capacity, counts, stream=0,
                           child_dirty=None):
        import torch
        self.branch_calls += 1
        st = status[:n].numpy()
        unk = np.nonzero(st == 2)[0]
        off = np.zeros(n + 1, np.int64) if excl_off is None else excl_off[:n + 1].numpy().astype(np.int64)
        lists = [excl.numpy()[off[i]:off[i + 1]] for i in unk]
        k = total = error = 0
        if len(unk):
            poff = np.concatenate([[0], np.cumsum([len(e) for e in lists])])
            pex = np.concatenate(lists).reshape(-1, 2)
            try:
                cl, cu, coff, cex, cd = S.branch_enumerate(lb[:n].numpy()[unk], ub[:n].numpy()[unk], poff, pex, val=val)
            except RuntimeError as e:
                error = 3 if "variable" in str(e).split(":")[0] else 4
            else:
                rows = [cex[coff[c]:coff[c + 1]] for c in range(len(cl))]
                if self._opts.get("branch_reverse"):
                    cl, cu, cd, rows = cl[::-1].copy(), cu[::-1].copy(), cd[::-1].copy(), rows[::-1]
                k, total = len(cl), sum(len(r) for r in rows)
                if total > capacity:
                    error = 1
                else:
                    child_lb[:k] = torch.from_numpy(cl)
                    child_ub[:k] = torch.from_numpy(cu)
                    if child_dirty is not None:
                        child_dirty[:k] = torch.from_numpy(cd)
                    child_excl_off[:k + 1] = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32))
                    if total:
                        child_excl[:total] = torch.from_numpy(np.concatenate(rows).astype(np.int32))
        counts[:] = torch.tensor([k, int((st == 1).sum()), int((st == 0).sum()), len(unk), int((st > 2).sum()), total, error, 0], dtype=counts.dtype)


def _root(n):
    return np.ones(n, np.int32), np.full(n, n, np.int32)


_REFERENCE = {}


def _reference_loop(n, val, node_limit=0):
    """(nodes, solutions, failures, sorted solutions): left-first DFS, one node at a time."""
    key = (n, val, node_limit)
    if key in _REFERENCE:
        return _REFERENCE[key]
    props = M.nqueens_props(n)
    lb0, ub0 = _root(n)
    stack = [(lb0, ub0, np.zeros((0, 2), np.int32))]
    nodes = sol = fail = 0
    sols = []
    while stack:
        L, U, ex = stack.pop()
        st, lb, ub = _consistency(n, props, L, U, ex)
        nodes += 1
        if node_limit and nodes >= node_limit:  # StopNode: the node that reaches the limit is a node and nothing else
            break
        if st == 0:
            fail += 1
        elif st == 1:
            sol += 1
            sols.append(tuple(int(x) for x in lb))
        else:
            cl, cu, coff, cex, _ = S.branch_enumerate(lb, ub, [0, len(ex)], ex, val=val)
            stack.append((cl[1], cu[1], cex[coff[1]:coff[2]].copy()))
            stack.append((cl[0], cu[0], cex[coff[0]:coff[1]].copy()))
    _REFERENCE[key] = (nodes, sol, fail, sorted(sols))
    return _REFERENCE[key]


def _search(n, val, batch, node_limit=0, **kw):
    import torch
    ctx = EnumOracleCtx(n, M.nqueens_props(n))
    ds = DeviceSearch(ctx, batch=batch, device=torch.device("cpu"), implicit=True, brancher="enumerate", val=val, **kw)
    st = ds.run(*_root(n), all_solutions=True, node_limit=node_limit, keep_solutions=1 << 20)
    return ds, ctx, (st.num_nodes, st.num_solution, st.num_failed_node, sorted(tuple(int(x) for x in s) for s in st.solutions))


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("n", [4, 5, 6, 7, 8])
def test_solution_counts_and_the_tree_at_every_batch_size(n, val, golden_dir):
    want = json.load(open(os.path.join(golden_dir, "engine_kats.json")))["search"]["all_solutions"]["counts"][n - 1]
    ref = _reference_loop(n, val)
    assert ref[1] == want and len(ref[3]) == want
    for batch in (1, 7, 64):
        ds, ctx, got = _search(n, val, batch)
        assert got == ref, (batch, got[:3], ref[:3])  # the tree does not depend on the order its nodes are taken in
        assert ctx.hints_seen == got[0] - 1  # every node but the root came with the variable it was branched on
        assert not ds.segs and not ds.esegs


@pytest.mark.parametrize("val", ["middle", "min"])
def test_small_buffers_merge_compact_and_take_fewer_nodes(val):
    """Rows and arena so small that segments are merged, the stack is compacted and rounds take fewer nodes than the batch: same tree."""
    n = 8
    ref = _reference_loop(n, val)
    ds, ctx, got = _search(n, val, 7, capacity=64, excl_capacity=48)
    assert got == ref
    ev = ds.arena_events
    assert ev["merge"] > 0 and ev["compact"] > 0, ev
    if val == "middle":
        assert ev["fewer"] > 0, ev
        # an arena that cannot hold one node's children: as for the row stack, an error
        with pytest.raises(RuntimeError, match="exclusion arena full"):
            _search(n, val, 7, capacity=64, excl_capacity=16)
    else:
        assert ev["fewer"] == 0  # MinVal's value is a bound: x != v always folds, no list is ever written
    with pytest.raises(RuntimeError, match="open-node stack full"):
        _search(n, val, 7, capacity=6)


@pytest.mark.parametrize("val", ["middle", "min"])
def test_stop_node_at_every_limit(val):
    n = 6
    size = _reference_loop(n, val)[0]
    assert size > 20
    for limit in range(1, size + 1):
        ref = _reference_loop(n, val, node_limit=limit)
        _, _, got = _search(n, val, 1, node_limit=limit)
        assert got == ref, (limit, got[:3], ref[:3])
        assert got[0] == limit


def test_max_rounds_stop_at_and_first_solution():
    import torch
    n, val = 6, "middle"
    ref = _reference_loop(n, val)
    ctx = EnumOracleCtx(n, M.nqueens_props(n))
    ds = DeviceSearch(ctx, batch=3, device=torch.device("cpu"), implicit=True, brancher="enumerate", val=val)
    ds.reset(*_root(n))
    assert not ds.advance(max_rounds=2) and ds.stats.rounds == 2
    assert not ds.advance(stop_at=11) and ds.stats.num_nodes == 11
    assert ds.advance(keep_solutions=2)
    assert (ds.stats.num_nodes, ds.stats.num_solution, ds.stats.num_failed_node) == ref[:3] and len(ds.stats.solutions) == 2
    one = DeviceSearch(ctx, batch=1, device=torch.device("cpu"), implicit=True, brancher="enumerate", val=val).run(*_root(n), all_solutions=False, keep_solutions=1)
    assert one.num_solution == 1 and tuple(int(x) for x in one.solutions[0]) in ref[3]


def test_refusals():
    import torch
    from pcp_amd import distributed as D
    n = 6
    ctx = EnumOracleCtx(n, M.nqueens_props(n))
    cpu = torch.device("cpu")
    kw = dict(batch=4, device=cpu, brancher="enumerate")
    with pytest.raises(ValueError, match="cells"):
        DeviceSearch(ctx, implicit=True, cells=True, **kw)
    with pytest.raises(ValueError, match="objective"):
        DeviceSearch(ctx, implicit=True, objective=(0, "min"), **kw)
    with pytest.raises(ValueError, match="implicit"):
        DeviceSearch(ctx, implicit=False, **kw)  # explicit `active` rows
    with pytest.raises(ValueError, match="val"):
        DeviceSearch(ctx, implicit=True, val="max", **kw)
    with pytest.raises(ValueError, match="brancher"):
        DeviceSearch(ctx, implicit=True, batch=4, device=cpu, brancher="input_order")
    sctx = EnumOracleCtx(n, M.nqueens_props(n))
    sctx.set_words = 1
    with pytest.raises(ValueError, match="set mode"):
        DeviceSearch(sctx, implicit=True, **kw)
    ds = DeviceSearch(ctx, implicit=True, **kw)
    ds.reset(*_root(n))
    with pytest.raises(ValueError, match="Enumerate"):
        D.parallel_search_device(ds, *_root(n), None)
    with pytest.raises(ValueError, match="Enumerate"):
        D.balance_stacks(ds, None)
    # the default is BinarySplit, as before
    assert DeviceSearch(ctx, batch=4, device=cpu, implicit=True).brancher == "split"
