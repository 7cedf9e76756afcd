"""The variable selector InputOrder (search/branching/input_order.rs:30-39; option "var_select" of the device) — TEST INFRASTRUCTURE shared by
the test_var_select_*.py files: a scalar restatement of the selector that shares no code with pcp_amd.search, rows built so that InputOrder
and FirstSmallestVar disagree, stand-in contexts that honour ``var_select`` (subclasses of the existing ones), the models the searches run
on, and their brute-force solution sets.  numpy only; nothing here touches a GPU."""
import functools
import itertools

import numpy as np

from pcp_amd import model as M
from pcp_amd import search as S

from enum_set_ref import SetOracleDeviceCtx
from oracle_ctx import OracleDeviceCtx
from test_enum_search_cpu import EnumOracleCtx
from test_form_excl_cpu import FormExclOracleCtx

BOUND_MAX = (1 << 29) - 1  # |bound| limit of int32 rows (PCP_BOUND_MAX): the widest domain has 2^30 - 1 values
WIDTHS = (1, 2, 63, 64, 65, 255, 256, 257, 300)  # the wave seam (64) and the 256-thread stride seam
FIRSTS = (0, 63, 64, 255, 256)                   # ... and V - 1: where the first open variable sits


# ---------------------------------------------------------------------------------------------------------------- the scalar selector
def ref_input_order(sizes):
    """The first index whose size is > 1, or None (the reference panics, input_order.rs:37).  Plain Python integers."""
    for i, s in enumerate(sizes):
        if int(s) > 1:
            return i
    return None


def ref_first_smallest(sizes):
    best = None
    for i, s in enumerate(sizes):
        if int(s) > 1 and (best is None or int(s) < int(sizes[best])):
            best = i
    return best


# ---------------------------------------------------------------------------------------------------------------- rows where the selectors disagree
def firsts_of(V):
    return sorted({f for f in FIRSTS if f < V} | {V - 1})


def interval_rows(V):
    """One row per position of the first open variable (firsts_of(V)): every variable before it assigned, the variable itself wide — up to
    2^30 - 1 values —, and, wherever a variable lies behind it, a strictly smaller open one at the LAST index (and a middling one right behind
    the first), so that FirstSmallestVar answers another index.  Returns (lb, ub [n, V] int32, first [n])."""
    rows = firsts_of(V)
    lb = np.zeros((len(rows), V), np.int32)
    ub = np.zeros((len(rows), V), np.int32)
    wide = [(-BOUND_MAX, BOUND_MAX), (-7, 1000), (0, BOUND_MAX), (-5, 4), (3, 40)]
    for r, f in enumerate(rows):
        lb[r] = ub[r] = np.arange(V) % 7 - 3  # assigned, each to some value
        lb[r, f], ub[r, f] = wide[r % len(wide)]
        if f + 1 < V:
            lb[r, V - 1], ub[r, V - 1] = 1, 2
        if f + 2 < V:
            lb[r, f + 1], ub[r, f + 1] = -1, 1
    return lb, ub, np.array(rows)


def set_rows(V, sw, base):
    """The same rows as sets over the hull [base, base + 64 sw): bits [n, V, sw] uint64, lb / ub [n, V]; the first open variable has holes."""
    rows = firsts_of(V)
    top = base + 64 * sw - 1
    sets = []
    for r, f in enumerate(rows):
        row = [[base + (v * 5) % (64 * sw)] for v in range(V)]
        row[f] = sorted({base, base + 3, base + 63 % (64 * sw), top - 2, top})
        if f + 1 < V:
            row[V - 1] = [base + 1, top]
        if f + 2 < V:
            row[f + 1] = [base, base + 2, top - 1]
        sets.append(row)
    bits = np.zeros((len(rows), V, sw), np.uint64)
    lb, ub = np.zeros((len(rows), V), np.int32), np.zeros((len(rows), V), np.int32)
    for i, row in enumerate(sets):
        for j, vals in enumerate(row):
            for v in vals:
                k, bit = divmod(int(v) - base, 64)
                bits[i, j, k] |= np.uint64(1) << np.uint64(bit)
            lb[i, j], ub[i, j] = min(vals), max(vals)
    return bits, lb, ub, np.array(rows)


def batch_of(n, n_rows):
    """A batch of n nodes drawn from n_rows rows in turn, statuses mixed by position (node 0 Unknown): (row index per node, status [n] uint8)."""
    idx = np.arange(n) % n_rows
    status = np.array([M.UNKNOWN, M.TRUE, M.UNKNOWN, M.FALSE, M.UNKNOWN], np.uint8)[np.arange(n) % 5]
    return idx, status


# ---------------------------------------------------------------------------------------------------------------- stand-in contexts
class VarSelectStandIn:
    """What a stand-in context gains: ``var_select`` as engine.Context has it (every assignment is logged in ``var_select_log``), the numpy
    branchers called with it, and ``set_option`` calls logged by key."""

    _var_select = "first_smallest"

    @property
    def var_select(self):
        return self._var_select

    @var_select.setter
    def var_select(self, name):
        assert name in ("first_smallest", "input_order"), name
        self.__dict__.setdefault("var_select_log", []).append(name)
        self._var_select = name

    def set_option(self, key, value):
        self.__dict__.setdefault("option_keys", []).append(key)
        super().set_option(key, value)


def _write_children(self, cl, cu, ca, L, U, child_lb, child_ub, child_active, child_dirty):
    import torch
    if self._opts.get("branch_reverse"):
        cl, cu, ca = cl[::-1].copy(), cu[::-1].copy(), (None if ca is None else ca[::-1].copy())
    k = cl.shape[0]
    if child_dirty is not None:
        pl_, pu_ = np.repeat(L, 2, axis=0), np.repeat(U, 2, axis=0)
        if self._opts.get("branch_reverse"):
            pl_, pu_ = pl_[::-1], pu_[::-1]
        child_dirty[:k] = torch.from_numpy(((cl != pl_) | (cu != pu_)).argmax(axis=1).astype(np.int32))
    child_lb[:k] = torch.from_numpy(cl)
    child_ub[:k] = torch.from_numpy(cu)
    if ca is not None:
        child_active[:k] = torch.from_numpy(ca.view(np.int64))
    return k


class VSOracleDeviceCtx(VarSelectStandIn, OracleDeviceCtx):
    """OracleDeviceCtx whose BinarySplit brancher is search.branch(var_select=ctx.var_select)."""

    def branch_device(self, n, lb, ub, active, status, child_lb, child_ub, child_active, counts, stream=0, child_dirty=None):
        import torch
        st = status[:n].numpy()
        unk = st == 2
        L, U = lb[:n].numpy()[unk], ub[:n].numpy()[unk]
        A = None if active is None else active[:n].numpy().view(np.uint64)[unk]
        k = 0
        if unk.any():
            k = _write_children(self, *S.branch(L, U, A, var_select=self.var_select), L, U, child_lb, child_ub, child_active, child_dirty)
        counts[:] = torch.tensor([k, int((st == 1).sum()), int((st == 0).sum()), int(unk.sum()), 0], dtype=counts.dtype)


def _branch_device_excl(self, n, lb, ub, status, excl_off, excl, val, child_lb, child_ub, child_excl_off, child_excl, capacity, counts, stream=0,
                        child_dirty=None):
    """EnumOracleCtx.branch_device_excl with the variable the context's selector names."""
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
        L, U = lb[:n].numpy()[unk], ub[:n].numpy()[unk]
        x = S.select_var(L, U, self.var_select)
        if (x < 0).any():
            error = 3
        else:
            cl, cu, coff, cex, cd = S.branch_enumerate(L, U, poff, pex, val=val, var=x)
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


class VSEnumOracleCtx(VarSelectStandIn, EnumOracleCtx):
    branch_device_excl = _branch_device_excl
    branch_device = VSOracleDeviceCtx.branch_device


class VSFormExclOracleCtx(VarSelectStandIn, FormExclOracleCtx):
    branch_device_excl = _branch_device_excl
    branch_device = VSOracleDeviceCtx.branch_device


class VSSetOracleDeviceCtx(VarSelectStandIn, SetOracleDeviceCtx):
    """SetOracleDeviceCtx whose two branchers take the variable the context's selector names."""

    def _branch_sets(self, n, bits, lb, ub, active, status, child_bits, child_active, counts, make):
        import torch
        st = status[:n].numpy()
        unk = st == 2
        k = 0
        if unk.any():
            B = bits[:n].numpy().view(np.uint64)[unk]
            A = None if active is None else active[:n].numpy().view(np.uint64)[unk]
            cb, ca = make(B, lb[:n].numpy()[unk], ub[:n].numpy()[unk], A)
            if self._opts.get("branch_reverse"):
                cb, ca = cb[::-1].copy(), (None if ca is None else ca[::-1].copy())
            k = len(cb)
            child_bits[:k] = torch.from_numpy(cb.view(np.int64))
            if ca is not None:
                child_active[:k] = torch.from_numpy(ca.view(np.int64))
        head = [k, int((st == 1).sum()), int((st == 0).sum()), int(unk.sum()), int((st > 2).sum())]
        counts[:] = torch.tensor((head + [0, 0, 0])[:len(counts)], dtype=counts.dtype)

    def branch_device_set(self, n, bits, lb, ub, active, status, child_bits, child_active, counts, stream=0):
        self._branch_sets(n, bits, lb, ub, active, status, child_bits, child_active, counts,
                          lambda B, L, U, A: S.branch_set(B, L, U, self._base_of(), A, var_select=self.var_select))

    def branch_device_set_enum(self, n, bits, lb, ub, active, status, val, child_bits, child_active, counts, stream=0):
        name = {0: "middle", 1: "min"}.get(val, val)
        self._branch_sets(n, bits, lb, ub, active, status, child_bits, child_active, counts,
                          lambda B, L, U, A: S.branch_enumerate_set(B, L, U, self._base_of(), A, val=name, var=S.select_var_set(B, self.var_select)))

    def _base_of(self):
        return self.base


# ---------------------------------------------------------------------------------------------------------------- models
@functools.lru_cache(maxsize=None)
def robot(num_robot=2, max_time=500):
    """(vs, cs, starts, durations, lb0, ub0, pushes, sums) of model.robot_scheduling."""
    vs, cs, starts, durations = M.robot_scheduling(num_robot, max_time)
    lb0, ub0 = vs.bounds()
    sums = []
    pushes = cs.pushes(len(vs), sums_out=sums)
    return vs, cs, starts, durations, lb0, ub0, pushes, sums


def push_store(target, n_vars, pushes, sums, set_words=0):
    """A lowered store on an engine Context or an OracleModel (what model.push_model does, from cached pushes)."""
    target.reset_model(n_vars, set_words)
    for members in sums:
        target.push_sum(members)
    for p in pushes:
        if p[0] == "props":
            target.push_props(p[1])
        else:
            target.push_formula(p[1], p[2])


ROBOT_PINNED = {"nodes": 60, "failed": 25, "starts": [1, 11, 36, 276, 301]}  # what restate_robot() gives on robot(2, 500): pinned by test_var_select_cpu.py


def brute_queens(n):
    """Every solution of N-queens n (values 1 .. n), sorted tuples."""
    return sorted(p for p in itertools.permutations(range(1, n + 1))
                  if all(abs(p[i] - p[j]) != j - i for i in range(n) for j in range(i + 1, n)))


# ---------------------------------------------------------------------------------------------------------------- any store, oracle-backed
class StoreOracleCtx(VarSelectStandIn, EnumOracleCtx):
    """A stand-in over ANY lowered store (vs, cs) — formula units, Sum views, plain propagators — for the host specifications: ``propagate``
    (search.dfs), ``propagate_device`` (DeviceSearch under BinarySplit) and the Enumerate round, whose nodes are judged by the oracle on the store
    plus one XNeqY(x, Constant(v)) behind it per entry (Branch::distribute, branch.rs:36-55).  It says ``has_formulas`` so that every
    Enumerate launch of the drivers is ``propagate_device_form_excl``; no objective.  One judgement per distinct node, shared."""

    def __init__(self, vs, cs):
        OracleDeviceCtx.__init__(self, len(vs), np.zeros(0, dtype=M.PROP_DTYPE))
        self._vs, self._cs = vs, cs
        self._sums = []
        self._pushes = cs.pushes(len(vs), sums_out=self._sums)
        self._m = self._model(())
        self.n_units, self.words = self._m.n_units, self._m.words
        self.has_formulas, self.all_neq = True, False
        self.branch_calls = self.form_calls = 0
        self._judged = {}

    def _model(self, ex):
        from oracle import oracle as orc
        om = orc.OracleModel(self.n_vars)
        push_store(om, self.n_vars, self._pushes, self._sums)
        if ex:
            p = np.zeros(len(ex), dtype=M.PROP_DTYPE)
            p["kind"] = M.NEQ
            p["var"][:] = [0, M.PCP_CONST, M.PCP_NOVAR]
            p["var"][:, 0] = [int(e[0]) for e in ex]
            p["off"][:, 1] = [int(e[1]) for e in ex]
            om.push_props(p)
        return om

    def judge(self, L, U, ex):
        """(status, lb, ub) of one node with the exclusions ex = [(var, value)]."""
        ex = tuple((int(a), int(b)) for a, b in ex)
        key = (L.tobytes(), U.tobytes(), ex)
        if key not in self._judged:
            r = (self._model(ex) if ex else self._m).consistency(L[None], U[None], None)
            self._judged[key] = (int(r[3][0]), r[0][0].copy(), r[1][0].copy())
        return self._judged[key]

    def propagate_device_excl(self, *a, **k):
        raise AssertionError("a store with formula units: pcp_propagate_device_form_excl is the entry")

    propagate_device_small_excl = propagate_device_excl

    def propagate_device_form_excl(self, n, lb_in, ub_in, lb_out, ub_out, active_out, status, excl_off, excl, objective=None, stream=0):
        import torch
        assert active_out is None and objective is None
        self.form_calls += 1
        L, U = lb_in[:n].numpy().copy(), ub_in[:n].numpy().copy()
        off, ex = excl_off[:n + 1].numpy(), excl.numpy()
        for i in range(n):
            st, lb, ub = self.judge(L[i], U[i], ex[off[i]:off[i + 1]])
            status[i] = st
            lb_out[i], ub_out[i] = torch.from_numpy(lb), torch.from_numpy(ub)
        self._stats["nodes"] += n

    branch_device_excl = _branch_device_excl
    branch_device = VSOracleDeviceCtx.branch_device


def restate_enumerate(ctx, lb0, ub0, var_of, first_only=True):
    """A plain pop / propagate / branch loop under Brancher<var_of, MinVal, Enumerate>, one node per step, written without pcp_amd.search's
    branchers: the left child x = lb(x) on top; the right child x != lb(x) folds into the lower bound (MinVal's value is always a bound, so no
    exclusion is ever carried).  ``var_of(sizes)`` names the variable (ref_input_order / ref_first_smallest).  Returns dict(nodes, failed,
    solutions, first = the first solution's lower bounds)."""
    stack = [(np.array(lb0, np.int32), np.array(ub0, np.int32))]
    r = {"nodes": 0, "failed": 0, "solutions": 0, "first": None}
    while stack:
        L, U = stack.pop()
        st, lb, ub = ctx.judge(L, U, ())
        r["nodes"] += 1
        if st == M.FALSE:
            r["failed"] += 1
        elif st == M.TRUE:
            r["solutions"] += 1
            if r["first"] is None:
                r["first"] = lb.copy()
            if first_only:
                break
        else:
            x = var_of([int(u) - int(l) + 1 for l, u in zip(lb, ub)])
            left = (lb.copy(), ub.copy()); right = (lb.copy(), ub.copy())
            left[1][x] = lb[x]
            right[0][x] = lb[x] + 1
            stack.append(right)
            stack.append(left)
    return r
