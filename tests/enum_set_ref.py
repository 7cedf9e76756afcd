"""Enumerate over IntervalSet stores — TEST INFRASTRUCTURE shared by test_enum_set_cpu.py and test_enum_set_gpu.py: oracle-backed set-mode
contexts (host-stepped and device-shaped, over CPU tensors) and the judge, a plain left-first DFS: one node at a time from a Python list,
OracleModel.consistency_set, pcp_amd.search.branch_enumerate_set.  Every tree is computed once, shared by the tests and never changed."""
import numpy as np

from oracle import oracle as orc
from pcp_amd import model as M
from pcp_amd import search as S

from oracle_ctx import OracleCtx, OracleDeviceCtx

SET_KINDS = [M.NEQ, M.EQ, M.LT, M.LT3, M.GT3, M.EQ3]  # the six propagator kinds set mode has (no XEqYMulZ over sets)


class SetOracleCtx(OracleCtx):
    """OracleCtx with the set-mode entry `propagate_set` that search.dfs_set / dfs_enumerate_set drive."""

    def __init__(self, n_vars, props, set_words, base):
        super().__init__(n_vars, props)
        self.set_words, self.base = set_words, base

    def propagate_set(self, bits, active=None, want_stats=True):
        lb, ub, b, act, st, s = self._m.consistency_set(bits, self.base, active)
        return lb, ub, b, act, st, {"steps": s["steps"], "steps3": 0}


class SetOracleDeviceCtx(OracleDeviceCtx):
    """OracleDeviceCtx in set mode, with the set brancher of the Enumerate round: propagate_device over `bits` rows is the oracle's
    consistency_set, branch_device_set_enum is search.branch_enumerate_set plus the counts of pcp_branch_device_set_enum."""

    def __init__(self, n_vars, props, set_words, base):
        super().__init__(n_vars, props)
        self.set_words, self.base = set_words, base
        self.supports_set_enumerate = True
        self.branch_calls = 0

    def propagate_device(self, n, lb_in, ub_in, lb_out, ub_out, active_in, active_out, status, stream=0, bits_in=None, bits_out=None, dirty=None, cells=False):
        import torch
        assert bits_in is not None and dirty is None and not cells
        B = bits_in[:n].numpy().view(np.uint64).copy()
        assert B.any(axis=2).all()  # (an Enumerate child is never empty)
        A = None if active_in is None else active_in[:n].numpy().view(np.uint64).copy()
        lb, ub, b, act, st, s = self._m.consistency_set(B, self.base, A)
        lb_out[:n], ub_out[:n] = torch.from_numpy(lb), torch.from_numpy(ub)
        bits_out[:n] = torch.from_numpy(b.view(np.int64))
        if active_out is not None:
            active_out[:n] = torch.from_numpy(act.view(np.int64))
        status[:n] = torch.from_numpy(st)
        self._stats["steps"] += s["steps"]
        self._stats["nodes"] += n

    def branch_device_set_enum(self, n, bits, lb, ub, active, status, val, child_bits, child_active, counts, stream=0):
        import torch
        self.branch_calls += 1
        st = status[:n].numpy()
        unk = np.nonzero(st == 2)[0]
        k = error = 0
        if len(unk):
            A = None if active is None else active[:n].numpy().view(np.uint64)[unk]
            try:
                cb, ca = S.branch_enumerate_set(bits[:n].numpy().view(np.uint64)[unk], lb[:n].numpy()[unk], ub[:n].numpy()[unk], self.base, A, val=val)
            except RuntimeError:
                error = 3
            else:
                if self._opts.get("branch_reverse"):
                    cb, ca = cb[::-1].copy(), (None if ca is None else ca[::-1].copy())
                k = len(cb)
                child_bits[:k] = torch.from_numpy(cb.view(np.int64))
                if ca is not None:
                    child_active[:k] = torch.from_numpy(ca.view(np.int64))
        counts[:] = torch.tensor([k, int((st == 1).sum()), int((st == 0).sum()), len(unk), int((st > 2).sum()), 0, error, 0], dtype=counts.dtype)


def nqueens_model(n, base=1):
    """(props, set_words, lb0, ub0) of N-queens as the reference allocates it (example/src/nqueens.rs:32-35)."""
    return M.nqueens_props(n), (n + 63) // 64, np.ones(n, np.int32), np.full(n, n, np.int32)


_TREES = {}


def reference_dfs(key, n_vars, props, root_bits, base, val, node_limit=0, first_only=False):
    """The judge.  Left-first DFS under Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate> below ``root_bits`` ([n_vars, set_words]),
    one oracle call per node.  Returns dict(nodes, solutions, failed, sols = the solutions sorted, first = the first solution or None).
    node_limit: the StopNode rule — the node that reaches the limit is a node and nothing else.  first_only: stop at the first solution.
    ``key`` names the model (the result is cached under it and the other arguments)."""
    ck = (key, np.ascontiguousarray(root_bits, np.uint64).tobytes(), base, val, node_limit, first_only)
    if ck in _TREES:
        return _TREES[ck]
    om = orc.OracleModel(n_vars, props)
    stack = [np.ascontiguousarray(root_bits, np.uint64).reshape(n_vars, -1)]
    nodes = sol = fail = 0
    sols, first = [], None
    while stack:
        lb, ub, b, _, st, _ = om.consistency_set(stack.pop()[None], base)
        nodes += 1
        if node_limit and nodes >= node_limit:
            break
        if st[0] == M.FALSE:
            fail += 1
        elif st[0] == M.TRUE:
            sol += 1
            sols.append(tuple(int(x) for x in lb[0]))
            if first is None:
                first = lb[0].copy()
            if first_only:
                break
        else:
            cb, _ = S.branch_enumerate_set(b, lb, ub, base, None, val=val)
            stack.append(cb[1])
            stack.append(cb[0])
    _TREES[ck] = {"nodes": nodes, "solutions": sol, "failed": fail, "sols": sorted(sols), "first": first}
    return _TREES[ck]


def nqueens_tree(n, val, node_limit=0, first_only=False):
    props, sw, lb0, ub0 = nqueens_model(n)
    return reference_dfs(("nqueens", n), n, props, M.interval_bits(lb0, ub0, sw, 1), 1, val, node_limit, first_only)
