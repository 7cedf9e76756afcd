"""Host-side search driver over the batched HIP engine — the *caller* side of the hot path.

The reference keeps the search tree on the host (north_star) and calls ``Space::consistency`` once per node
(search/propagation.rs:42-55).  This driver keeps that structure but hands the engine many open nodes per
call.  Branching follows the reference's default engine (search/mod.rs:45-52):

* variable  ``FirstSmallestVar``  (search/branching/first_smallest_var.rs:30-39): first index among the
  variables of minimal size > 1;
* value     ``MiddleVal``         (search/branching/middle_val.rs:25-27): (lb+ub)/2, truncating toward zero;
* split     ``BinarySplit``       (search/branching/binary_split.rs:33-60): children ``x <= v`` and ``x > v``.

A branch constraint is a var-vs-constant ``XLessY`` that narrows its one variable on its first run and is then
entailed and unlinked (x_less_y.rs:87-93, propagation/store.rs:171), so it is folded into the child's bounds
(SURVEY.md §8b "per-node propagators"); children inherit the parent's ``active`` row, exactly the cstore label
``(len, active.clone())`` of propagation/store.rs:315-317.

Branch and bound (``objective=(var, "min" | "max")``, search/branch_and_bound.rs:64-84): once a solution is known every node
entered gets one more unary propagator, ``var < best`` (Minimize) or ``var > best`` (Maximize); it narrows ``var`` once and
is then entailed, so it is folded into the node's domain before propagation like a branch constraint.  A Satisfiable node
makes ``var.lower()`` the incumbent (both modes).  With a batch, every node of the batch is folded against the incumbent as
it stands, and the best Satisfiable node of the batch (ties: the first in pop order) replaces it if it beats it.  The
search then runs to the end (the reference's AllSolution<OneSolution<BranchAndBound<..>>>).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from .engine import full_active
from .model import FALSE, TRUE, UNKNOWN, interval_bits


def first_smallest_var(lb: np.ndarray, ub: np.ndarray) -> np.ndarray:
    """Row-wise FirstSmallestVar.  Rows where every variable is assigned return -1 (the reference panics)."""
    size = ub.astype(np.int64) - lb.astype(np.int64) + 1
    big = np.iinfo(np.int64).max
    key = np.where(size > 1, size, big)
    idx = key.argmin(axis=1)  # argmin returns the FIRST minimum, as min_by_key does
    none = key[np.arange(key.shape[0]), idx] == big
    return np.where(none, -1, idx)


def input_order(lb: np.ndarray, ub: np.ndarray) -> np.ndarray:
    """Row-wise InputOrder (search/branching/input_order.rs:30-39): the first variable in store order whose size is > 1.  Rows where every
    variable is assigned return -1 (the reference panics, input_order.rs:37)."""
    return _first_open(ub.astype(np.int64) - lb.astype(np.int64) + 1)


def input_order_set(bits: np.ndarray) -> np.ndarray:
    """InputOrder on sets (bits: [n, V, set_words]): the first variable of CARDINALITY > 1; -1 where there is none."""
    return _first_open(_popcount64(bits).sum(axis=2))


def _first_open(size: np.ndarray) -> np.ndarray:
    size = size.reshape(1, -1) if size.ndim == 1 else size
    open_ = size > 1
    return np.where(open_.any(axis=1), open_.argmax(axis=1), -1)  # argmax: the FIRST True


VAR_SELECTORS = ("first_smallest", "input_order")


def _check_var_select(var_select: str) -> str:
    if var_select not in VAR_SELECTORS:
        raise ValueError(f"var_select must be 'first_smallest' or 'input_order', not {var_select!r}")
    return var_select


def select_var(lb: np.ndarray, ub: np.ndarray, var_select: str = "first_smallest") -> np.ndarray:
    """The variable selector by name on Interval rows: first_smallest_var or input_order."""
    return (input_order if _check_var_select(var_select) == "input_order" else first_smallest_var)(lb, ub)


def select_var_set(bits: np.ndarray, var_select: str = "first_smallest") -> np.ndarray:
    """The variable selector by name on set-mode rows, sizes being cardinalities; -1 where every variable is assigned."""
    if _check_var_select(var_select) == "input_order":
        return input_order_set(bits)
    size = _popcount64(bits).sum(axis=2)
    return first_smallest_var(np.ones_like(size), size)  # (FirstSmallestVar on sizes: ub - lb + 1 = the cardinality)


def middle_val(lb: np.ndarray, ub: np.ndarray) -> np.ndarray:
    s = lb.astype(np.int64) + ub.astype(np.int64)
    return (np.sign(s) * (np.abs(s) // 2)).astype(np.int32)  # Rust `/` truncates toward zero


def branch(lb: np.ndarray, ub: np.ndarray, active: Optional[np.ndarray], var_select: str = "first_smallest"):
    """BinarySplit children of each (Unknown) row, folded: returns (lb2, ub2, active2) with 2 rows per input row,
    ordered left child then right child.  ``var_select``: FirstSmallestVar's variable or InputOrder's."""
    n = lb.shape[0]
    var = select_var(lb, ub, var_select)
    if (var < 0).any():
        raise RuntimeError("Cannot select a variable in a space where all variables are assigned.")
    rows = np.arange(n)
    v = middle_val(lb[rows, var], ub[rows, var])
    L = np.repeat(lb, 2, axis=0)
    U = np.repeat(ub, 2, axis=0)
    U[2 * rows, var] = np.minimum(U[2 * rows, var], v)          # x <= v
    L[2 * rows + 1, var] = np.maximum(L[2 * rows + 1, var], v + 1)  # x > v
    A = None if active is None else np.repeat(active, 2, axis=0)
    return L, U, A


@dataclass
class SearchStats:
    num_nodes: int = 0
    num_solution: int = 0
    num_failed_node: int = 0
    launches: int = 0
    filter_steps: int = 0
    solutions: List[np.ndarray] = field(default_factory=list)
    best: Optional[int] = None                  # branch and bound: the incumbent (None: no solution)
    best_solution: Optional[np.ndarray] = None  # the lb row of the node that set it
    incumbents: List[int] = field(default_factory=list)  # every improvement, in order


def _objective(objective):
    """(var, "min" | "max") -> (var, minimize?) or None."""
    if objective is None:
        return None
    var, mode = objective
    if mode not in ("min", "max"):
        raise ValueError(f"objective mode must be 'min' or 'max', not {mode!r}")
    return int(var), mode == "min"


def _improve(st: SearchStats, obj, lb: np.ndarray, status: np.ndarray):
    """The reduce of a propagated batch: the Satisfiable row with the best lb[var] (ties: the lowest row) becomes the incumbent if it
    beats it."""
    var, minimize = obj
    rows = np.nonzero(status == TRUE)[0]
    if not len(rows):
        return
    vals = lb[rows, var].astype(np.int64)
    r = rows[vals.argmin() if minimize else vals.argmax()]  # argmin / argmax: the first of equal values
    v = int(lb[r, var])
    if st.best is None or (v < st.best if minimize else v > st.best):
        st.best = v
        st.best_solution = lb[r].copy()
        st.incumbents.append(v)


def bfs_frontier(ctx, lb0: np.ndarray, ub0: np.ndarray, n_open: int, max_rounds: int = 64, active0: Optional[np.ndarray] = None,
                 implicit: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray, SearchStats]:
    """Expand the search tree breadth-first until at least ``n_open`` open (branched, not yet propagated) nodes
    exist; returns their folded (lb, ub, active) rows, at most ``n_open`` of them, in tree order.  ``lb0/ub0`` may be
    one root or a block of open nodes (with their ``active0`` rows) to continue from.  ``implicit``: nodes are domains
    only (no `active` rows; the engine derives liveness from the domains, include/pcp_hip.h) and A is None."""
    from .engine import full_active
    st = SearchStats()
    L = np.ascontiguousarray(lb0, np.int32)
    L = L.reshape(1, -1) if L.ndim == 1 else L
    U = np.ascontiguousarray(ub0, np.int32).reshape(L.shape)
    if implicit:
        A = None
    else:
        A = full_active(L.shape[0], ctx.n_units) if active0 is None else np.ascontiguousarray(active0, np.uint64).reshape(L.shape[0], -1)
    for _ in range(max_rounds):
        if L.shape[0] >= n_open or L.shape[0] == 0:
            break
        ok = (L <= U).all(axis=1)  # a folded branch can be empty: that child is failed without a launch
        st.num_failed_node += int((~ok).sum())
        L, U, A = L[ok], U[ok], (None if A is None else A[ok])
        if L.shape[0] == 0:
            break
        lb, ub, act, status, s = ctx.propagate(L, U, A)
        st.launches += 1
        st.num_nodes += L.shape[0]
        st.filter_steps += s["steps"] + s["steps3"]
        st.num_failed_node += int((status == FALSE).sum())
        for r in np.nonzero(status == TRUE)[0]:
            st.num_solution += 1
            st.solutions.append(lb[r].copy())
        unk = status == UNKNOWN
        L, U, A = branch(lb[unk], ub[unk], None if act is None else act[unk])
    ok = (L <= U).all(axis=1)
    return L[ok][:n_open], U[ok][:n_open], (None if A is None else A[ok][:n_open]), st


def _search(kind, root, all_solutions: bool, node_limit: int, batch: int, obj=None, rows_up: bool = False) -> SearchStats:
    """The depth-first loop of dfs / dfs_set / dfs_enumerate over a LIFO stack of open nodes.  ``kind`` says what a node is:
    ``kind.propagate(st, take, obj)`` stacks the popped nodes, propagates them (counting launches and filter steps in ``st``) and returns
    (lb rows, status, the propagated batch); ``kind.branch(batch, unk)`` returns the children of its rows ``unk``: two nodes per row, left then right.
    ``rows_up``: a batch is the top ``batch`` nodes in the order of their rows on DeviceSearch's stack, the lowest first — the children of the
    LOWEST Unknown node end on top, a tie between solutions goes to the lowest, the node that reaches a limit is the lowest.  Under branch and
    bound the order in which the nodes of a batch are entered decides what the next batch is bounded by, so a host specification of
    DeviceSearch(objective=) has to take them as it does; with batch = 1 both orders are the reference's."""
    st = SearchStats()
    all_solutions = all_solutions or obj is not None
    stack = [root]
    while stack:
        take = stack[-batch:] if rows_up else stack[-batch:][::-1]  # top of the stack first (rows_up: last)
        del stack[-batch:]
        if node_limit:
            left = max(0, node_limit - st.num_nodes)
            take = take[len(take) - min(left, len(take)):] if rows_up else take[:left]  # the `left` nodes nearest the top
            if not take:
                break
        lb, status, done_batch = kind.propagate(st, take, obj)
        st.num_nodes += len(take)
        at_limit = bool(node_limit and st.num_nodes >= node_limit)
        if at_limit:
            # StopNode hands EndOfSearch to the monitor for the node that reaches the limit (stop_node.rs:57-62 under Monitor,
            # stop_node.rs:90-97): it is counted as a node, never as a solution or a failure
            status[0 if rows_up else -1] = UNKNOWN
        st.num_failed_node += int((status == FALSE).sum())
        true = np.nonzero(status == TRUE)[0]
        st.num_solution += len(true)
        st.solutions += [lb[r].copy() for r in true]
        if obj is not None:
            _improve(st, obj, lb, status)
        if (len(true) and not all_solutions) or at_limit:
            break
        unk = np.nonzero(status == UNKNOWN)[0]
        if len(unk):
            # push so that the first taken node's left child ends on top: the parents in reverse, right then left
            stack += kind.branch(done_batch, unk)[::-1]
    return st


class _IntervalRows:
    """A node is (lb, ub, active).  The incumbent is folded into the bounds; a node with lb > ub is failed without a launch."""

    def __init__(self, ctx, var_select="first_smallest"):
        self.ctx, self.var_select = ctx, _check_var_select(var_select)

    def propagate(self, st, take, obj):
        L, U, A = (np.stack(c) for c in zip(*take))
        if obj is not None and st.best is not None:  # the bound propagator, folded
            if obj[1]:
                U[:, obj[0]] = np.minimum(U[:, obj[0]], st.best - 1)
            else:
                L[:, obj[0]] = np.maximum(L[:, obj[0]], st.best + 1)
        ok = (L <= U).all(axis=1)
        status = np.zeros(L.shape[0], np.uint8)
        if ok.any():
            L[ok], U[ok], A[ok], status[ok], s = self.ctx.propagate(L[ok], U[ok], A[ok])
            st.launches += 1
            st.filter_steps += s["steps"] + s["steps3"]
        return L, status, (L, U, A)

    def branch(self, done_batch, unk):
        return list(zip(*branch(*(a[unk] for a in done_batch), var_select=self.var_select)))


def dfs(ctx, lb0: np.ndarray, ub0: np.ndarray, all_solutions: bool = False, node_limit: int = 0, batch: int = 1, objective=None,
        var_select: str = "first_smallest") -> SearchStats:
    """Depth-first search with a LIFO stack of open nodes (gcollections::VectorStack in the reference).  With
    ``batch=1`` the node order is exactly the reference's left-first DFS (one_solution.rs:46-51, 92-105); with
    ``batch>1`` the top ``batch`` open nodes are propagated in one launch (batched subtree propagation).
    ``objective=(var, "min" | "max")``: branch and bound on that variable (module docstring); the search runs to the end
    whatever ``all_solutions`` says, and ``best`` / ``best_solution`` / ``incumbents`` of the result report it.
    ``var_select="input_order"``: InputOrder instead of FirstSmallestVar (the host specification of option var_select of the device)."""
    _check_var_select(var_select)
    obj = _objective(objective)
    root = (np.ascontiguousarray(lb0, np.int32), np.ascontiguousarray(ub0, np.int32), full_active(1, ctx.n_units)[0])
    return _search(_IntervalRows(ctx, var_select), root, all_solutions, node_limit, batch, obj)


# ---------------------------------------------------------------------------------------------------------------------
# Enumerate (search/branching/enumerate.rs:33-60): children ``x = v`` and ``x != v``.  ``x = v`` folds into the child's bounds like a
# BinarySplit constraint.  ``x != v`` on an Interval removes v only at a bound (x_neq_y.rs:82-93): with v AT a bound it fires once and is then
# entailed — folded —, with v inside the domain it removes nothing and stays in that node's cstore: the child carries the exclusion
# (x, v) and the engine propagates it with the model (pcp_propagate_device_excl).  Exclusions are int32 [m, 2] arrays of (var, value) pairs
# — the bytes of pcp_excl — in CSR form: node i owns excl[excl_off[i] : excl_off[i + 1]].
# ---------------------------------------------------------------------------------------------------------------------
def _excl_pairs(excl) -> np.ndarray:
    if excl is None:
        return np.zeros((0, 2), np.int32)
    e = np.asarray(excl)
    if e.dtype.names:  # a structured (var, value) array
        e = np.stack([e["var"].astype(np.int64), e["value"].astype(np.int64)], axis=1) if len(e) else np.zeros((0, 2), np.int64)
    return np.ascontiguousarray(e, np.int32).reshape(-1, 2)


def branch_enumerate(lb: np.ndarray, ub: np.ndarray, excl_off=None, excl=None, val: str = "middle", var=None):
    """Enumerate children of each (Unknown, propagated) row: returns (L, U, off, excl2, dirty) with 2 rows per input row, ``x = v`` first
    (the reference's order, enumerate.rs:47-60).  The variable is FirstSmallestVar's (``var``: an index or one per row instead — the
    reference's test_distributor distributes on a given variable); the value MiddleVal's (``val="middle"``) or MinVal's (``"min"``:
    dom.lower(), min_val.rs:25-27).  Left child: x = v in the bounds.  Right child: the exclusion (x, v) appended behind the inherited ones,
    or, when v is a bound of x, folded into that bound (the propagator would fire once and be entailed: the same fixpoint).  Both children
    inherit those of the parent's exclusions whose value still lies inside their variable's domain IN THE CHILD (the others are entailed for
    good: domains only shrink).  ``dirty``: the variable branched on — each child differs from its parent's fixpoint in it alone.
    One departure from the letter of the reference: an interior x != v leaves an Interval as it is, so the right child is its parent again and
    MiddleVal would choose the same v for ever (the reference's Enumerate tests use MinVal, whose value is a bound and always goes).  A value
    the node has excluded already is therefore not chosen again: the nearest value to it that is still free is taken, the lower one first."""
    if val not in ("middle", "min"):
        raise ValueError(f"val must be 'middle' or 'min', not {val!r}")
    lb = np.ascontiguousarray(lb, np.int32)
    lb = lb.reshape(1, -1) if lb.ndim == 1 else lb
    ub = np.ascontiguousarray(ub, np.int32).reshape(lb.shape)
    n = lb.shape[0]
    pairs = _excl_pairs(excl)
    off = np.zeros(n + 1, np.int64) if excl_off is None else np.asarray(excl_off, np.int64)
    rows = np.arange(n)
    x = first_smallest_var(lb, ub) if var is None else np.broadcast_to(np.asarray(var, np.int64), (n,))
    if (x < 0).any() or (lb[rows, x] >= ub[rows, x]).any():
        raise RuntimeError("Cannot select a variable in a space where all variables are assigned.")
    v = middle_val(lb[rows, x], ub[rows, x]) if val == "middle" else lb[rows, x].copy()
    for i in range(n):  # a value this node has excluded already is not tried again (see the docstring)
        taken = {int(w) for y, w in pairs[off[i]:off[i + 1]] if y == x[i]}
        if int(v[i]) in taken:
            lo, hi = int(lb[i, x[i]]), int(ub[i, x[i]])
            # (outwards from v, stopping at the first free value: at most 2 * len(taken) + 2 candidates are looked at, whatever the width)
            free = next((c for d in range(1, hi - lo + 1) for c in (int(v[i]) - d, int(v[i]) + d) if lo <= c <= hi and c not in taken), None)
            if free is None:
                raise RuntimeError("Cannot select a value: every value of the variable is excluded.")
            v[i] = free
    L = np.repeat(lb, 2, axis=0)
    U = np.repeat(ub, 2, axis=0)
    L[2 * rows, x] = v; U[2 * rows, x] = v  # x = v
    at_lb, at_ub = v == lb[rows, x], v == ub[rows, x]
    L[2 * rows + 1, x] = np.where(at_lb, v + 1, lb[rows, x])  # x != v with v at a bound
    U[2 * rows + 1, x] = np.where(at_ub & ~at_lb, v - 1, ub[rows, x])
    out, off2 = [], [0]
    for i in range(n):
        mine = pairs[off[i]:off[i + 1]]
        for c in (2 * i, 2 * i + 1):
            keep = mine[(mine[:, 1] >= L[c, mine[:, 0]]) & (mine[:, 1] <= U[c, mine[:, 0]])] if len(mine) else mine
            if c & 1 and not (at_lb[i] or at_ub[i]):
                keep = np.concatenate([keep, np.array([[x[i], v[i]]], np.int32)])
            out.append(keep)
            off2.append(off2[-1] + len(keep))
    excl2 = np.ascontiguousarray(np.concatenate(out), np.int32).reshape(-1, 2) if out else np.zeros((0, 2), np.int32)
    return L, U, np.asarray(off2, np.int32), excl2, np.repeat(x, 2).astype(np.int32)


class _ExclRows:
    """A node is (lb, ub, exclusions [k, 2], dirty variable), propagated on torch tensors through ``ctx.propagate_device_excl`` (an all-XNeqY
    model without an objective), ``ctx.propagate_device_small_excl`` (``small``: any other small store, and every search with an objective) or
    ``ctx.propagate_device_form_excl`` (a context that says ``has_formulas``: a store with formula units, with or without an objective).
    The children of branch_enumerate are never empty; with an objective the incumbent is folded into the bounds here, as _IntervalRows does,
    and a node the fold empties is failed without a launch."""

    def __init__(self, ctx, val, record, hints, small=False, var_select="first_smallest"):
        import torch
        self.var_select = _check_var_select(var_select)
        self.torch, self.ctx, self.val, self.record, self.hints, self.small = torch, ctx, val, record, hints, small
        self.form = bool(getattr(ctx, "has_formulas", False))  # a store with formula units: ctx.propagate_device_form_excl, whatever `small` says
        on_gpu = getattr(ctx, "device", 0) != "cpu"  # (the CPU tests drive this class with an oracle-backed stand-in context)
        self.dev = torch.device("cuda", ctx.device) if on_gpu else torch.device("cpu")
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream if on_gpu else 0

    def propagate(self, st, take, obj):
        L, U = (np.stack([t[i] for t in take]) for i in (0, 1))
        if obj is None or st.best is None:
            return self._launch(st, take, L, U)
        if obj[1]:  # the bound propagator, folded
            U[:, obj[0]] = np.minimum(U[:, obj[0]], st.best - 1)
        else:
            L[:, obj[0]] = np.maximum(L[:, obj[0]], st.best + 1)
        ok = np.nonzero((L <= U).all(axis=1))[0]
        lb, ub, status = L.copy(), U.copy(), np.zeros(L.shape[0], np.uint8)
        if len(ok):
            lb[ok], status[ok], (_, ub[ok], _) = self._launch(st, [take[i] for i in ok], L[ok], U[ok])
        return lb, status, (lb, ub, take)

    def _launch(self, st, take, L, U):
        torch, dev = self.torch, self.dev
        N = L.shape[0]
        off = np.zeros(N + 1, np.int32)
        off[1:] = np.cumsum([len(t[2]) for t in take])
        flat = np.concatenate([t[2] for t in take]).astype(np.int32).reshape(-1, 2)
        t_lb, t_ub = torch.from_numpy(L.copy()).to(dev), torch.from_numpy(U.copy()).to(dev)
        t_st = torch.zeros(N, dtype=torch.uint8, device=dev)
        t_off = torch.from_numpy(off).to(dev)
        t_ex = torch.from_numpy(flat if len(flat) else np.zeros((1, 2), np.int32)).to(dev)  # (never a null pointer: an empty list is offsets alone)
        t_dirty = torch.tensor([t[3] for t in take], dtype=torch.int32, device=dev) if (self.hints and not self.small and not self.form) else None
        if self.form:
            self.ctx.propagate_device_form_excl(N, t_lb, t_ub, t_lb, t_ub, None, t_st, t_off, t_ex, None, self.stream)
        elif self.small:
            self.ctx.propagate_device_small_excl(N, t_lb, t_ub, t_lb, t_ub, None, t_st, t_off, t_ex, None, self.stream)
        else:
            self.ctx.propagate_device_excl(N, t_lb, t_ub, t_lb, t_ub, None, t_st, t_off, t_ex, self.stream, dirty=t_dirty)
        lb, ub, status = t_lb.cpu().numpy(), t_ub.cpu().numpy(), t_st.cpu().numpy()
        st.launches += 1
        if (status > UNKNOWN).any():
            raise RuntimeError("dfs_enumerate: the engine refused a node (PCP_STATUS_HULL)")
        if self.record is not None:
            self.record += [(L[i].copy(), U[i].copy(), take[i][2].copy(), int(status[i]), lb[i].copy(), ub[i].copy()) for i in range(N)]
        return lb, status, (lb, ub, take)

    def branch(self, done_batch, unk):
        lb, ub, take = done_batch
        poff = np.zeros(len(unk) + 1, np.int64)
        poff[1:] = np.cumsum([len(take[u][2]) for u in unk])
        pex = np.concatenate([take[u][2] for u in unk]).reshape(-1, 2)
        x = None if self.var_select == "first_smallest" else input_order(lb[unk], ub[unk])  # (-1: branch_enumerate raises)
        cl, cu, coff, cex, cd = branch_enumerate(lb[unk], ub[unk], poff, pex, val=self.val, var=x)
        return [(cl[c], cu[c], cex[coff[c]:coff[c + 1]].copy(), int(cd[c])) for c in range(len(cl))]


def dfs_enumerate(ctx, lb0: np.ndarray, ub0: np.ndarray, all_solutions: bool = False, node_limit: int = 0, batch: int = 1, val: str = "middle",
                  record: Optional[list] = None, hints: bool = True, objective=None, var_select: str = "first_smallest") -> SearchStats:
    """The batched host-stepped depth-first search of ``dfs`` under Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate>: the top
    ``batch`` open nodes go through ``ctx.propagate_device_excl`` in one launch, each with its own exclusions (and, with ``hints``, the
    variable it was branched on as its dirty-variable hint).  ``record``: a list that receives, per node in the order propagated,
    (lb_in, ub_in, exclusions [k, 2], status, lb_out, ub_out).
    A model that is not all-XNeqY (``ctx.all_neq``) — a small store of any plain propagators, the Golomb network — goes through
    ``ctx.propagate_device_small_excl`` instead (no hints: that kernel sweeps a node as a whole).  So does every search with an
    ``objective`` (as in dfs: BranchAndBound wraps any brancher, branch_and_bound.rs:64-84) — unless the context says ``has_formulas`` (a store
    with formula units, a schedule): then every launch is ``ctx.propagate_device_form_excl``.  The bound is folded into a node's bounds before
    its propagation exactly as under BinarySplit; this is the host specification of DeviceSearch(brancher="enumerate", objective=), so a
    batch is taken in the order of DeviceSearch's rows (``rows_up`` of _search): the same nodes, solutions, failures and incumbents at every
    batch size.  ``var_select="input_order"``: Brancher<InputOrder, ..> — the brancher of the reference's scheduling examples with ``val="min"``."""
    _check_var_select(var_select)
    obj = _objective(objective)
    small = obj is not None or not getattr(ctx, "all_neq", True)
    kind, V = _ExclRows(ctx, val, record, hints, small, var_select), ctx.n_vars
    steps0 = ctx.stats_read(kind.stream)
    root = (np.ascontiguousarray(lb0, np.int32).reshape(V), np.ascontiguousarray(ub0, np.int32).reshape(V), np.zeros((0, 2), np.int32), -1)
    st = _search(kind, root, all_solutions, node_limit, batch, obj, rows_up=obj is not None)
    steps1 = ctx.stats_read(kind.stream)
    st.filter_steps = (steps1["steps"] + steps1["steps3"]) - (steps0["steps"] + steps0["steps3"])  # over the whole call, not per launch
    return st


# ---------------------------------------------------------------------------------------------------------------------
# Set mode (IntervalSet<i32> domains as bitsets — the reference's default FDSpace, search/mod.rs:41-43).  The same engine,
# with the selectors the reference applies to sets: FirstSmallestVar compares CARDINALITIES (first_smallest_var.rs:30-39:
# `v.size()`), MiddleVal is (lower + upper) / 2 (middle_val.rs:25-27), BinarySplit keeps the values <= v resp. > v.
# ---------------------------------------------------------------------------------------------------------------------
def _popcount64(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.uint64)
    m1, m2, m4 = np.uint64(0x5555555555555555), np.uint64(0x3333333333333333), np.uint64(0x0F0F0F0F0F0F0F0F)
    a = a - ((a >> np.uint64(1)) & m1)
    a = (a & m2) + ((a >> np.uint64(2)) & m2)
    a = (a + (a >> np.uint64(4))) & m4
    return ((a * np.uint64(0x0101010101010101)) >> np.uint64(56)).astype(np.int64)


def branch_set(bits: np.ndarray, lb: np.ndarray, ub: np.ndarray, base: int, active: Optional[np.ndarray], var_select: str = "first_smallest"):
    """BinarySplit children of each (Unknown) set-mode row, folded into the sets: returns (bits2, active2), 2 rows per input
    row (left `x <= v`, then right `x > v`).  bits: [n, V, set_words]; lb/ub: the sets' bounds."""
    from .model import interval_bits
    n, V, sw = bits.shape
    var = select_var_set(bits, var_select)
    rows = np.arange(n)
    if (var < 0).any():
        raise RuntimeError("Cannot select a variable in a space where all variables are assigned.")
    v = middle_val(lb[rows, var], ub[rows, var]).astype(np.int64)
    B = np.repeat(bits, 2, axis=0)
    lo_mask = interval_bits(np.full(n, base, np.int64), v, sw, base)                      # values <= v
    hi_mask = interval_bits(v + 1, np.full(n, base + 64 * sw - 1, np.int64), sw, base)    # values > v
    B[2 * rows, var] &= lo_mask
    B[2 * rows + 1, var] &= hi_mask
    A = None if active is None else np.repeat(active, 2, axis=0)
    return B, A


class _Sets:
    """A node is (bits, active or None).  The incumbent is folded through interval_bits; a node with an emptied set is failed without a launch."""

    def __init__(self, ctx, base, implicit, var_select="first_smallest"):
        self.ctx, self.base, self.implicit, self.var_select = ctx, base, implicit, _check_var_select(var_select)

    def propagate(self, st, take, obj):
        sw, base = self.ctx.set_words, self.base
        Bt = np.stack([t[0] for t in take])
        A = None if self.implicit else np.stack([t[1] for t in take])
        if obj is not None and st.best is not None:
            top = base + 64 * sw - 1
            keep = interval_bits(base, min(st.best - 1, top), sw, base) if obj[1] else interval_bits(max(st.best + 1, base), top, sw, base)
            Bt[:, obj[0]] &= keep
        ok = Bt.any(axis=2).all(axis=1)
        status = np.zeros(Bt.shape[0], np.uint8)
        lb = np.ones(Bt.shape[:2], np.int32); ub = np.zeros(Bt.shape[:2], np.int32)
        if ok.any():
            lb[ok], ub[ok], Bt[ok], pact, status[ok], s = self.ctx.propagate_set(Bt[ok], None if A is None else A[ok])
            if A is not None:
                A[ok] = pact
            st.launches += 1
            st.filter_steps += s["steps"] + s["steps3"]
        return lb, status, (Bt, lb, ub, A)

    def branch(self, done_batch, unk):
        Bt, lb, ub, A = done_batch
        cb, ca = branch_set(Bt[unk], lb[unk], ub[unk], self.base, None if A is None else A[unk], var_select=self.var_select)
        return [(cb[c], None if ca is None else ca[c]) for c in range(len(cb))]


def dfs_set(ctx, lb0: np.ndarray, ub0: np.ndarray, base: int, all_solutions: bool = False, node_limit: int = 0, batch: int = 1,
            implicit: bool = True, objective=None, var_select: str = "first_smallest") -> SearchStats:
    """Depth-first search over set-mode nodes (FDSpace): the variables are allocated as IntervalSet::new(lb0, ub0)
    (example/src/nqueens.rs:32-35); with batch = 1 the node order is the reference's left-first DFS.  ``objective``: as in dfs;
    the bound clears the objective's values >= best (min) or <= best (max) from its set.  ``var_select``: as in dfs, on cardinalities."""
    _check_var_select(var_select)
    obj = _objective(objective)
    root = (interval_bits(np.asarray(lb0), np.asarray(ub0), ctx.set_words, base), None if implicit else full_active(1, ctx.n_units)[0])
    return _search(_Sets(ctx, base, implicit, var_select), root, all_solutions, node_limit, batch, obj)


# ---------------------------------------------------------------------------------------------------------------------
# Enumerate over sets (search/branching/enumerate.rs:33-60 on FDSpace).  On an IntervalSet XEqY(x, Constant v) intersects x with {v}
# and XNeqY(x, Constant v) removes v wherever it sits; both are then entailed.  So both children fold into the variable's set: no
# exclusion lists, and the propagation is dfs_set's.  The value rule is DESIGN.md §2 "Value selection on a set".
# ---------------------------------------------------------------------------------------------------------------------
def set_members(words: np.ndarray, base: int) -> np.ndarray:
    """The values of one variable's set (words: [set_words] uint64, value v = bit v - base), ascending."""
    w = np.ascontiguousarray(words, np.uint64).reshape(-1)
    on = (w[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    return np.nonzero(on.reshape(-1))[0].astype(np.int64) + int(base)


def enumerate_value_set(words: np.ndarray, lo: int, hi: int, base: int, val: str = "middle") -> int:
    """The value Enumerate branches a set on.  MinVal: lo (min_val.rs:25-27).  MiddleVal: m = (lo + hi) / 2 truncated toward zero
    (middle_val.rs:25-27).  The value taken is the member of the set nearest to that, m - d before m + d: m itself whenever it is a member
    (always, for MinVal on the set's own lower bound), otherwise — where the reference would branch on an absent value for ever — the
    nearest one."""
    if val not in ("middle", "min"):
        raise ValueError(f"val must be 'middle' or 'min', not {val!r}")
    s = int(lo) + int(hi)
    m = int(lo) if val == "min" else (abs(s) // 2) * (1 if s >= 0 else -1)
    mem = set_members(words, base)
    if not len(mem):
        raise RuntimeError("Cannot select a value: the variable's set is empty.")
    key = 2 * np.abs(mem - m) + (mem > m)
    return int(mem[key.argmin()])


def branch_enumerate_set(bits: np.ndarray, lb: np.ndarray, ub: np.ndarray, base: int, active: Optional[np.ndarray], val: str = "middle", var=None):
    """Enumerate children of each (Unknown, propagated) set-mode row, folded into the sets: returns (bits2, active2), 2 rows per input row,
    ``x = v`` (the variable's set becomes {v}) then ``x != v`` (bit v cleared) — the reference's order, enumerate.rs:47-60.  The variable is
    FirstSmallestVar's on cardinalities (``var``: an index or one per row instead, as the reference's test_distributor distributes); the value
    is enumerate_value_set's on the row's bounds lb / ub.  Neither child is ever empty: the variable has two values or more and v is one of
    them.  Everything else is copied.  This is the specification pcp_branch_device_set_enum is compared with."""
    if val not in ("middle", "min"):
        raise ValueError(f"val must be 'middle' or 'min', not {val!r}")
    bits = np.ascontiguousarray(bits, np.uint64)
    bits = bits[None] if bits.ndim == 2 else bits
    n, V, sw = bits.shape
    lb = np.asarray(lb).reshape(n, V)
    ub = np.asarray(ub).reshape(n, V)
    size = _popcount64(bits).sum(axis=2)
    rows = np.arange(n)
    if var is None:
        big = np.iinfo(np.int64).max
        key = np.where(size > 1, size, big)
        x = key.argmin(axis=1)
    else:
        x = np.broadcast_to(np.asarray(var, np.int64), (n,))
    if n and (size[rows, x] <= 1).any():
        raise RuntimeError("Cannot select a variable in a space where all variables are assigned.")
    B = np.repeat(bits, 2, axis=0)
    for i in range(n):
        v = enumerate_value_set(bits[i, x[i]], lb[i, x[i]], ub[i, x[i]], base, val)
        k, bit = divmod(v - int(base), 64)
        one = np.uint64(1) << np.uint64(bit)
        B[2 * i, x[i]] = 0
        B[2 * i, x[i], k] = one        # x = v
        B[2 * i + 1, x[i], k] &= ~one  # x != v
    A = None if active is None else np.repeat(active, 2, axis=0)
    return B, A


class _SetsEnumerate(_Sets):
    """_Sets under Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate>."""

    def __init__(self, ctx, base, implicit, val, var_select="first_smallest"):
        super().__init__(ctx, base, implicit, var_select)
        self.val = val

    def branch(self, done_batch, unk):
        Bt, lb, ub, A = done_batch
        x = None if self.var_select == "first_smallest" else input_order_set(Bt[unk])
        if x is not None and (x < 0).any():
            raise RuntimeError("Cannot select a variable in a space where all variables are assigned.")
        cb, ca = branch_enumerate_set(Bt[unk], lb[unk], ub[unk], self.base, None if A is None else A[unk], val=self.val, var=x)
        return [(cb[c], None if ca is None else ca[c]) for c in range(len(cb))]


def dfs_enumerate_set(ctx, lb0: np.ndarray, ub0: np.ndarray, base: int, all_solutions: bool = False, node_limit: int = 0, batch: int = 1,
                      val: str = "middle", implicit: bool = True, objective=None, var_select: str = "first_smallest") -> SearchStats:
    """dfs_set under Enumerate: the same nodes, propagated by the same ``ctx.propagate_set``, branched by branch_enumerate_set.  With
    batch = 1 the node order is the reference's left-first DFS under Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate>.
    ``objective``: as in dfs_set — BranchAndBound wraps any brancher (branch_and_bound.rs:64-84), so the bound is folded into a node's
    set before its propagation exactly as under BinarySplit; this is the host specification of pcp_dfs_forest_device_set_bnb's Enumerate loop."""
    if val not in ("middle", "min"):
        raise ValueError(f"val must be 'middle' or 'min', not {val!r}")
    _check_var_select(var_select)
    obj = _objective(objective)
    root = (interval_bits(np.asarray(lb0), np.asarray(ub0), ctx.set_words, base), None if implicit else full_active(1, ctx.n_units)[0])
    return _search(_SetsEnumerate(ctx, base, implicit, val, var_select), root, all_solutions, node_limit, batch, obj)
