"""Device-resident subtree search: the open-node stack, propagation AND branching stay on the GPU; only four
counters per round cross PCIe ("removes the host round-trip per node").

Per round: the top ``batch`` open nodes of the stack are propagated in place (`pcp_propagate_device`), every Unknown
node is branched on the device (`pcp_branch_device`: FirstSmallestVar / MiddleVal / BinarySplit, folded, children
inherit the parent's `active` row), the batch is popped and the children are pushed.  With ``batch=1`` the node order
is exactly the reference's left-first DFS (search/engine/one_solution.rs:46-51, 92-105).
With ``objective=(var, "min" | "max")`` the round propagates through `pcp_propagate_device_bnb` instead (branch and bound,
search/branch_and_bound.rs:64-84): the incumbent stays on the device, is folded into every node of the batch before the fixpoint
and replaced by the batch's best Satisfiable node after it; it comes back in the same copy as the counts.
With ``brancher="enumerate"`` the round is `pcp_propagate_device_excl` + `pcp_branch_device_excl` (Brancher<FirstSmallestVar, MiddleVal | MinVal,
Enumerate>, search/branching/enumerate.rs:33-60): every open node owns a list of value exclusions, the lists live in a device arena next to the
rows and are written by the brancher — rows, hints and lists stay on the GPU from the root to the leaves.  A model that is not all-XNeqY (a
small store of any plain propagators: the Golomb network) and every Enumerate search with an ``objective`` propagate through
`pcp_propagate_device_small_excl` instead: the same lists on the one-wavefront-per-node kernel, the incumbent folded as a node is staged and
reduced behind the launch (no hints: that kernel sweeps a node as a whole).  A store with formula units (a schedule; ``ctx.has_formulas``)
takes `pcp_propagate_device_form_excl` in that place: the same call on the one-wavefront-per-node tree kernel.  Over a set-mode context the same
``brancher="enumerate"`` needs none of that: x = v and x != v are exact operations on the sets, so the round is `pcp_propagate_device` +
`pcp_branch_device_set_enum` on the rows of the BinarySplit search (no arena, no hints).
PyTorch provides the device buffers; every kernel is this repository's.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from .model import FALSE, TRUE


@dataclass
class DeviceSearchStats:
    num_nodes: int = 0
    num_solution: int = 0
    num_failed_node: int = 0
    rounds: int = 0
    filter_steps: int = 0
    evaluated: int = 0
    max_open: int = 0
    solutions: List[np.ndarray] = field(default_factory=list)
    best: Optional[int] = None                  # branch and bound: the incumbent (None: no solution)
    best_solution: Optional[np.ndarray] = None  # the lb row of the node that set it
    incumbents: List[int] = field(default_factory=list)  # every improvement, one per round at most


def _cut(t, lo: int, hi=None):
    """t[lo:hi] of a buffer the search may not keep (None)."""
    return None if t is None else t[lo:hi]


class _Int32Rows:
    """The node kind of a DeviceSearch: the buffers only it needs, the two engine calls of a round, and what happens to its side structures when
    segments are merged, the stack is compacted, a batch is popped and children are pushed (nothing, but for Enumerate).
    This one: int32 rows (lb, ub), with or without `active` rows, hints and an objective."""
    n_counts = 5  # round_buf: the brancher's counts[5], then (branch and bound) the incumbent and the improvement count

    def __init__(self, s):
        self.s = s

    def _nothing(self, *args): pass
    # the hooks of a kind with side structures: a new search starts; the top segment (l2 rows) was moved behind the one below (l1 rows); the
    # segments are about to become one; the round's buffer has arrived; its parents were popped (emptied: the top segment's last); its children pushed
    reset = merge = compact = check = pop = push = _nothing

    def take(self, n: int, final: bool = True) -> int: return n  # how many of the top n nodes a round may take (final: it is about to be launched)

    def unpacked(self, rows, stream):
        return rows

    def launch(self, n, lo, top, status, stream):
        s, ctx = self.s, self.s.ctx
        lb, ub, act = s.lb[lo:top], s.ub[lo:top], _cut(s.act, lo, top)
        if s.objective is None:
            ctx.propagate_device(n, lb, ub, lb, ub, act, act, status, stream, dirty=_cut(s.dirty, lo, top))
        else:
            ctx.propagate_device_bnb(n, lb, ub, lb, ub, act, act, status, s._obj, stream)
        ctx.branch_device(n, lb, ub, act, status, s.lb[top:], s.ub[top:], _cut(s.act, top), s.counts, stream, child_dirty=_cut(s.dirty, top))


class _Cells(_Int32Rows):
    """Rows of packed cells: `lb` holds the cells, there is no `ub`."""

    def unpacked(self, rows, stream):
        return self.s.ctx.unpack_rows(rows.contiguous(), stream_ptr=stream)[0]

    def launch(self, n, lo, top, status, stream):
        s, ctx = self.s, self.s.ctx
        ctx.propagate_device(n, s.lb[lo:top], None, s.lb[lo:top], None, None, None, status, stream, dirty=_cut(s.dirty, lo, top), cells=True)
        ctx.branch_device_cells(n, s.lb[lo:top], status, s.lb[top:], s.counts, stream, child_dirty=_cut(s.dirty, top))


class _Sets(_Int32Rows):
    """Sets (`bits`), with or without an objective; lb / ub receive the sets' bounds."""

    def launch(self, n, lo, top, status, stream):
        s, ctx = self.s, self.s.ctx
        lb, ub, act, bits = s.lb[lo:top], s.ub[lo:top], _cut(s.act, lo, top), s.bits[lo:top]
        if s.objective is None:
            ctx.propagate_device(n, None, None, lb, ub, act, act, status, stream, bits_in=bits, bits_out=bits)
        else:
            ctx.propagate_device_bnb(n, None, None, lb, ub, act, act, status, s._obj, stream, bits_in=bits, bits_out=bits)
        ctx.branch_device_set(n, bits, lb, ub, act, status, s.bits[top:], _cut(s.act, top), s.counts, stream)


class _SetsEnumerate(_Sets):
    """Sets under Enumerate: the round of _Sets with the other brancher (x = v / x != v folded into the sets)."""
    n_counts = 8  # round_buf: the brancher's counts[8]

    def launch(self, n, lo, top, status, stream):
        s, ctx = self.s, self.s.ctx
        lb, ub, act, bits = s.lb[lo:top], s.ub[lo:top], _cut(s.act, lo, top), s.bits[lo:top]
        ctx.propagate_device(n, None, None, lb, ub, act, act, status, stream, bits_in=bits, bits_out=bits)
        ctx.branch_device_set_enum(n, bits, lb, ub, act, status, s.val, s.bits[top:], _cut(s.act, top), s.counts, stream)

    def check(self, buf):
        if buf[6]:
            raise RuntimeError({3: "Cannot select a variable in a space where all variables are assigned."}.get(buf[6], f"pcp_branch_device_set_enum: error {buf[6]}"))


class _Enumerate(_Int32Rows):
    """Rows with exclusion lists.  The exclusion arena is managed like the row buffer.  Segment i of `segs` (rows [s, s + l)) owns
    esegs[i] = [o, e0, n, m]: its l + 1 offsets eoff[o : o + l + 1] (relative to e0, the first one 0) and the contiguous run of entries
    ex[e0 : e0 + n]; m bounds the entries of any ONE of its nodes (a child has at most one more than its parent).  A round writes the children's
    entries above the top segment's, their offsets above its offsets; the popped parents leave holes that are reclaimed with the rows (LIFO)."""
    n_counts = 8  # round_buf: the brancher's counts[8] and, behind them, the entries the top segment keeps after the pop

    def __init__(self, s, excl_capacity: int):
        self.s, torch = s, s.torch
        # A round over n nodes that own k entries writes at most 2 k + n entries (include/pcp_hip.h): the default holds as many bytes as the rows.
        s.ecap = int(excl_capacity) if excl_capacity else s.cap * max(s.V, 16)
        s.ex = torch.empty((s.ecap + 1, 2), dtype=torch.int32, device=s.dev)  # (+ 1: no slice of it is empty)
        s.eoff = torch.zeros(2 * s.cap + 4, dtype=torch.int32, device=s.dev)  # (a segment's o is at most twice its s)
        s.esegs = []
        s.arena_events = {"merge": 0, "compact": 0, "fewer": 0}

    def reset(self):
        self.s.eoff[0:2] = 0  # the root has no exclusions
        self.s.esegs = [[0, 0, 0, 0]]

    def merge(self, l1, l2):
        """The moved rows' entries go behind the lower segment's, their offsets (relative to the run's start) grow by its count."""
        s = self.s
        o2, e2, n2, m2 = s.esegs.pop()
        o1, e1, n1, m1 = s.esegs[-1]
        s._move(s.ex, e1 + n1, e2, n2)
        s.eoff[o1 + l1 + 1:o1 + l1 + 1 + l2] = s.eoff[o2 + 1:o2 + l2 + 1] + n1
        s.esegs[-1] = [o1, e1, n1 + n2, max(m1, m2)]
        s.arena_events["merge"] += 1

    def compact(self, segs):
        s = self.s
        pos = epos = emax = 0
        for i, ((_, l), (o, e0, cnt, m)) in enumerate(zip(segs, s.esegs)):
            s._move(s.ex, epos, e0, cnt)
            if i == 0:
                s._move(s.eoff, 0, o, l + 1)
            else:
                s.eoff[pos + 1:pos + l + 1] = s.eoff[o + 1:o + l + 1] + epos
            pos, epos, emax = pos + l, epos + cnt, max(emax, m)
        s.esegs = [[0, 0, epos, emax]] if pos else []
        s.arena_events["compact"] += 1

    def take(self, n, final=True):
        """As for the rows: what the children's lists may need has to fit above the top segment's entries."""
        s = self.s
        fit = s._arena_take(n)
        if not final or fit == n:
            return fit
        fit = s._arena_take(n, exact=True)
        if fit < 1:
            raise RuntimeError(f"exclusion arena full ({s.esegs[-1][1] + s.esegs[-1][2]} of {s.ecap} entries in use); raise `excl_capacity`")
        s.arena_events["fewer"] += fit < n
        return fit

    def launch(self, n, lo, top, status, stream):
        s, ctx = self.s, self.s.ctx
        (start, length), (o, e0, cnt, emax) = s.segs[-1], s.esegs[-1]
        k = lo - start  # the batch's first row within its segment
        lb, ub, poff, pex, etop, oc = s.lb[lo:top], s.ub[lo:top], s.eoff[o + k:o + length + 1], s.ex[e0:], e0 + cnt, o + length + 1
        if s.enum_form:
            ctx.propagate_device_form_excl(n, lb, ub, lb, ub, None, status, poff, pex, None if s.objective is None else s._obj, stream)
        elif s.enum_small:
            ctx.propagate_device_small_excl(n, lb, ub, lb, ub, None, status, poff, pex, None if s.objective is None else s._obj, stream)
        else:
            ctx.propagate_device_excl(n, lb, ub, lb, ub, None, status, poff, pex, stream, dirty=_cut(s.dirty, lo, top))
        ctx.branch_device_excl(n, lb, ub, status, poff, pex, s.val, s.lb[top:], s.ub[top:], s.eoff[oc:], s.ex[etop:], s.ecap - etop, s.counts, stream,
                               child_dirty=_cut(s.dirty, top))
        s.round_buf[8:9].copy_(s.eoff[o + k:o + k + 1])  # where the popped nodes' entries begin: what the segment keeps
        self.children = [oc, etop, emax + 1]  # the children's segment, should there be any

    def check(self, buf):
        if buf[6]:
            raise RuntimeError({1: "the exclusion arena was sized too small for this round", 3: "Cannot select a variable in a space where all variables are assigned.",
                                4: "Cannot select a value: every value of the variable is excluded."}.get(buf[6], f"pcp_branch_device_excl: error {buf[6]}"))

    def pop(self, buf, emptied):
        self.s.esegs[-1][2] = buf[8]
        if emptied:
            self.s.esegs.pop()

    def push(self, buf):
        oc, etop, m = self.children
        self.s.esegs.append([oc, etop, buf[5], m])


class DeviceSearch:
    """The open nodes live in one device buffer of ``capacity`` rows as a list of SEGMENTS (start, length), the last
    one on top.  A round propagates the top ``n`` rows of the last segment in place and lets `pcp_branch_device` write
    the children straight above them, in reverse order, as a new segment: nothing is copied or reordered.  The popped
    parents leave a hole below the new segment; it is reclaimed when that segment is used up (LIFO)."""

    def __init__(self, ctx, batch: int = 1024, capacity: int = 0, device=None, implicit: bool = False, hints=None, cells: bool = False, objective=None,
                 brancher: str = "split", val: str = "middle", excl_capacity: int = 0, var_select=None):
        import torch
        self.torch, self.ctx, self.batch = torch, ctx, int(batch)
        # var_select: None leaves the context's variable selector as it is; "first_smallest" / "input_order" is the context's selector (option
        # "var_select") while advance() runs, the value before restored afterwards.  (The selector is not a brancher: brancher= names the distributor.)
        if var_select is not None and var_select not in ("first_smallest", "input_order"):
            raise ValueError(f"var_select must be 'first_smallest' or 'input_order', not {var_select!r}")
        if cells and var_select == "input_order":
            raise ValueError("var_select='input_order' is not served by the packed-cell brancher (pcp_branch_device_cells selects FirstSmallestVar only): cells=True is refused")
        self.var_select = var_select
        # brancher="enumerate": children x = v / x != v instead of BinarySplit's x <= v / x > v; val: MiddleVal or MinVal (Enumerate only)
        if brancher not in ("split", "enumerate"):
            raise ValueError(f"brancher must be 'split' or 'enumerate', not {brancher!r}")
        self.brancher, self.val = brancher, val
        if brancher == "enumerate":
            if val not in ("middle", "min"):
                raise ValueError(f"val must be 'middle' or 'min', not {val!r}")
            if cells:
                raise ValueError("Enumerate runs on int32 rows: cells=True is refused")
            if objective is not None and getattr(ctx, "set_words", 0):
                raise ValueError("Enumerate takes no objective in set mode (branch and bound runs under BinarySplit there; forest_bnb_set(brancher=\"enumerate\") is the set-mode column)")
            if objective is not None and not getattr(ctx, "has_formulas", False) and not hasattr(ctx, "propagate_device_small_excl"):
                raise ValueError("Enumerate with an objective needs a context that offers propagate_device_small_excl (pcp_propagate_device_small_excl): this one does not")
            if getattr(ctx, "set_words", 0) and not getattr(ctx, "supports_set_enumerate", False):
                raise ValueError("Enumerate in set mode needs a context that offers branch_device_set_enum (pcp_branch_device_set_enum): this one does not")
            if not implicit and ctx.words:
                raise ValueError("Enumerate needs implicit nodes (pcp_propagate_device_excl takes no `active` rows)")
        self.dev = device if device is not None else torch.device("cuda", ctx.device)
        self.V, self.W = V, W = ctx.n_vars, max(ctx.words, 1)
        self.cap = int(capacity) if capacity else 8 * self.batch + 64
        i32, i64, u8 = torch.int32, torch.int64, torch.uint8
        # cells: the open nodes are rows of packed cells (pcp_device_batch.cell_format PCP_CELLS_PACKED16; all-XNeqY models with a declared hull
        # within +-16383, implicit nodes): `lb` holds the cells, there is no `ub` — half the bytes per open node, same search node for node
        self.cells = bool(cells)
        if self.cells and (not implicit or getattr(ctx, "set_words", 0)):
            raise ValueError("cells=True needs implicit nodes in interval mode")
        # objective=(var, "min" | "max"): branch and bound (pcp_propagate_device_bnb); the search then always runs to the end
        self.objective = None
        if objective is not None:
            var, mode = objective
            if mode not in ("min", "max"):
                raise ValueError(f"objective mode must be 'min' or 'max', not {mode!r}")
            if self.cells:
                raise ValueError("branch and bound runs on int32 rows: cells=True cannot take an objective")
            if not 0 <= int(var) < ctx.n_vars:
                raise ValueError(f"objective variable {var} is not a variable of the model")
            self.objective = (int(var), mode)
        self.lb = torch.empty((self.cap, V), dtype=i32, device=self.dev)
        self.ub = None if self.cells else torch.empty((self.cap, V), dtype=i32, device=self.dev)
        # implicit: a node record is its domains only — no `active` rows are kept, the engine derives liveness from the
        # domains (a node that descends from an all-active root has active = not entailed)
        self.implicit = bool(implicit) or not ctx.words
        self.act = None if self.implicit else torch.empty((self.cap, W), dtype=i64, device=self.dev)
        # set mode (IntervalSet domains, the reference's FDSpace): the node is its sets; lb/ub hold the sets' bounds after
        # propagation (the brancher's MiddleVal reads them)
        self.set_words = int(getattr(ctx, "set_words", 0))
        self.base = 0
        self.bits = torch.empty((self.cap, V, self.set_words), dtype=i64, device=self.dev) if self.set_words else None
        # one hint per open node (pcp_device_batch.dirty_var): a child is its parent's fixpoint with ONE variable branched on, so the engine
        # may start the child's propagation from that variable alone; the root has none (-1).  Interval mode, implicit nodes, an engine
        # that knows the field (the CPU stand-in of the tests does not).
        # Enumerate on pcp_propagate_device_small_excl: an objective, or a model that is not all-XNeqY (a context that does not say is taken as all-XNeqY)
        # Enumerate on pcp_propagate_device_form_excl: a store with formula units, with or without an objective (the rows, the arena and the round
        # buffer are enum_small's: only the propagate call differs)
        self.enum_form = brancher == "enumerate" and not self.set_words and bool(getattr(ctx, "has_formulas", False))
        self.enum_small = brancher == "enumerate" and not self.set_words and (self.objective is not None or self.enum_form or not getattr(ctx, "all_neq", True))
        want = bool(getattr(ctx, "supports_hints", False)) and self.implicit and not self.set_words and self.objective is None and not self.enum_small  # (bnb, small stores: no hints)
        self.dirty = torch.full((self.cap,), -1, dtype=i32, device=self.dev) if (want if hints is None else (hints and want)) else None
        self.status = torch.zeros(self.batch, dtype=u8, device=self.dev)
        self.segs: List[List[int]] = []  # [start, length], bottom to top
        self.stats = DeviceSearchStats()
        self.kind = ((_SetsEnumerate(self) if self.set_words else _Enumerate(self, excl_capacity)) if brancher == "enumerate"
                     else _Cells(self) if self.cells else _Sets(self) if self.set_words else _Int32Rows(self))
        # what a round brings back, side by side: its one copy to the host reads all of it
        # (under Enumerate words 5 .. 8 are the brancher's and the arena's: the incumbent and the improvement count follow them)
        self._ibest = 9 if (self.objective is not None and self.kind.n_counts > 5) else 5
        self.round_buf = torch.zeros(max(9, self._ibest + 2), dtype=i32, device=self.dev)
        self.counts = self.round_buf[:self.kind.n_counts]
        if self.objective is not None:
            self.best, self.improved = self.round_buf[self._ibest:self._ibest + 1], self.round_buf[self._ibest + 1:self._ibest + 2]
            self.best_lb, self.best_ub = torch.zeros(V, dtype=i32, device=self.dev), torch.zeros(V, dtype=i32, device=self.dev)
            self.best_bits = torch.zeros((V, self.set_words), dtype=i64, device=self.dev) if self.set_words else None
            self._obj = {"var": self.objective[0], "mode": self.objective[1], "best": self.best, "best_lb": self.best_lb, "best_ub": self.best_ub,
                         "best_bits": self.best_bits, "improved": self.improved}

    # ---- the stack as the drivers see it ------------------------------------------------------------------------------
    @property
    def size(self) -> int:
        return sum(l for _, l in self.segs)

    @size.setter
    def size(self, n: int):
        """Rows [0, n) are the open nodes (used by balance_stacks after it has moved rows around a compacted stack)."""
        self.segs = [[0, int(n)]] if n > 0 else []

    def _stream(self) -> int:
        """The HIP stream the engine is launched on (torch's current stream of this GPU; 0 off the GPU: the CPU tests drive
        this class with an oracle-backed stand-in context)."""
        return self.torch.cuda.current_stream(self.dev).cuda_stream if self.dev.type == "cuda" else 0

    def _rows(self):
        return tuple(t for t in (self.lb, self.ub, self.act, self.dirty, self.bits) if t is not None)

    @staticmethod
    def _move(t, dst: int, src: int, k: int):
        """t[dst : dst + k] = t[src : src + k] for dst <= src (the ranges may overlap)."""
        if k and dst != src:
            t[dst:dst + k] = t[src:src + k].clone() if src < dst + k else t[src:src + k]

    def _arena_take(self, n: int, exact: bool = False) -> int:
        """Enumerate: how many of the top segment's n top nodes the arena can branch in one round (their children's entries go above the
        segment's); 0 when not even one fits.  From what the host knows — the segment's entries and a bound on one node's —, or, ``exact``,
        from the segment's offsets (a copy from the device: only a round that the bound turns away pays it; it also renews the bound)."""
        o, e0, cnt, m = self.esegs[-1]
        room = self.ecap - (e0 + cnt)
        if 2 * min(cnt, n * m) + n <= room:
            return n
        if not exact:
            return min(n, room // (2 * m + 1))
        l = self.segs[-1][1]
        off = self.eoff[o:o + l + 1].cpu().numpy().astype(np.int64)
        self.esegs[-1][3] = int(np.diff(off).max())
        while n and 2 * int(off[l] - off[l - n]) + n > room:
            n -= 1
        return n

    def _merge_top(self, want: int):
        """Close the holes under the top segments until the top segment holds `want` nodes (or is the only one): only
        the small segments on top are moved, never the bulk of the stack."""
        while len(self.segs) > 1 and self.segs[-1][1] < want:
            s2, l2 = self.segs.pop()
            s1, l1 = self.segs[-1]
            for t in self._rows():
                self._move(t, s1 + l1, s2, l2)
            self.segs[-1][1] = l1 + l2
            self.kind.merge(l1, l2)

    def compact(self):
        """Make the open nodes one segment starting at row 0 (order kept)."""
        if len(self.segs) == 1 and self.segs[0][0] == 0:
            return
        self.kind.compact(self.segs)
        pos = 0
        for s, l in self.segs:
            for t in self._rows():
                self._move(t, pos, s, l)
            pos += l
        self.segs = [[0, pos]] if pos else []

    def reset(self, lb0, ub0, base: int = 0):
        """Start a new search: the stack holds the root (set mode: the variables as IntervalSet::new(lb0, ub0), value v = bit
        v - base, base = the hull's lower bound declared on the context)."""
        torch, ctx = self.torch, self.ctx
        from .engine import full_active, no_incumbent
        from .model import interval_bits
        self.solutions_ub = []  # advance(keep_bounds=True): the upper bounds of stats.solutions, row for row
        self.solutions_bits = []  # advance(keep_bits=True): the sets of stats.solutions, row for row ([V, set_words] uint64 each)
        if self.bits is not None:
            self.base = int(base)
            self.bits[0] = torch.from_numpy(interval_bits(np.asarray(lb0), np.asarray(ub0), self.set_words, self.base).view(np.int64)).to(self.dev)
        l0, u0 = (torch.from_numpy(np.ascontiguousarray(b, np.int32)).to(self.dev) for b in (lb0, ub0))
        if self.cells:
            ctx.pack_rows(l0.reshape(1, -1), u0.reshape(1, -1), self.lb[0:1], self._stream())
        else:
            self.lb[0], self.ub[0] = l0, u0
        if self.act is not None:
            self.act[0] = torch.from_numpy(full_active(1, ctx.n_units).view(np.int64)[0]).to(self.dev)
        if self.dirty is not None:
            self.dirty[0] = -1  # the root is propagated from scratch
        self.segs = [[0, 1]]
        self.stats = DeviceSearchStats()
        self.kind.reset()
        if self.objective is not None:
            self.best.fill_(no_incumbent(self.objective[1]))
            self.improved.zero_()
            self._improved_seen = 0
        ctx.stats_reset(self._stream())

    def advance(self, all_solutions: bool = True, node_limit: int = 0, max_rounds: int = 0, keep_solutions: int = 0, batch: int = 0, stop_at: int = 0,
                keep_bounds: bool = False, keep_bits: bool = False) -> bool:
        """Run rounds on the current stack until it is empty, a limit is hit, or (not all_solutions) a solution is
        found.  Returns True when the search is over (stack empty or solution found).
        ``node_limit`` is the search's StopNode limit (stop_node.rs:47-62): the node that reaches it is counted as a node and as nothing
        else.  ``stop_at`` only ends this call after that many nodes in total (a caller's chunk of a larger budget, e.g. one rank's share
        between two exchanges of parallel_search_device): every node's status counts.
        With an objective, ``all_solutions`` is ignored: branch and bound runs to the end of the search.
        ``keep_bounds`` (int32 rows only): every solution kept in ``stats.solutions`` also leaves its upper bounds in ``self.solutions_ub``, row
        for row (a True node of an interval store is a box; ``stats.solutions`` holds its lower corner, and the stats keep their fields).
        ``keep_bits`` (set mode only): the same for IntervalSet stores — a True node is a product of sets, and every solution kept also leaves
        its sets in ``self.solutions_bits``.
        A DeviceSearch built with ``var_select=`` runs them under that variable selector (engine.var_select_scope)."""
        from .engine import var_select_scope
        with var_select_scope(self.ctx, self.var_select):
            return self._advance(all_solutions, node_limit, max_rounds, keep_solutions, batch, stop_at, keep_bounds, keep_bits)

    def _advance(self, all_solutions, node_limit, max_rounds, keep_solutions, batch, stop_at, keep_bounds, keep_bits=False) -> bool:
        torch, ctx, st, kind = self.torch, self.ctx, self.stats, self.kind
        bnb = self.objective is not None
        all_solutions = all_solutions or bnb
        stream = self._stream()
        batch = min(int(batch) if batch else self.batch, self.batch)
        first_round, done = st.rounds, False
        ctx.set_option("branch_reverse", 1)  # children arrive in pop order (a context-wide knob: restored below)
        while self.segs:
            if max_rounds and st.rounds - first_round >= max_rounds:
                break
            self._merge_top(batch)
            start, length = self.segs[-1]
            top = start + length
            # the children (at most 2n rows, and for Enumerate their lists) go right above the popped parents: when a buffer is nearly full,
            # first squeeze out the holes, then take fewer nodes (a deeper, narrower dive) instead of overflowing
            want = min(batch, length)
            if self.cap - top < 2 * want or kind.take(want, final=False) < want:
                self.compact()
                start, length = self.segs[-1]
                top = start + length
            room = self.cap - top
            if room < 2:
                raise RuntimeError(f"open-node stack full ({self.size} of {self.cap}); raise `capacity`")
            n = kind.take(min(batch, length, room // 2))
            n = min([n] + [cap_nodes - st.num_nodes for cap_nodes in (node_limit, stop_at) if cap_nodes])
            if n <= 0:
                break
            lo = top - n
            status = self.status[:n]
            kind.launch(n, lo, top, status, stream)
            buf = self.round_buf.cpu().tolist()  # the round's only D2H sync
            n_children, n_true, n_false, _, n_other = buf[:5]
            if n_other:
                raise RuntimeError(f"{n_other} nodes were refused by the engine (bounds outside the declared hull): the search cannot continue")
            kind.check(buf)
            if bnb and buf[self._ibest + 1] != self._improved_seen:
                self._improved_seen = buf[self._ibest + 1]
                st.best = buf[self._ibest]
                st.incumbents.append(buf[self._ibest])
            st.rounds += 1
            st.num_nodes += n
            s_last = None
            if node_limit and st.num_nodes >= node_limit:
                # the node that reaches the limit (the last one in pop order: the lowest row of the round) is counted as a node, never as a
                # solution or a failure: StopNode hands EndOfSearch to the monitor (stop_node.rs:57-62 under Monitor, stop_node.rs:90-97)
                s_last = int(status[0].item())
                n_true, n_false = n_true - (s_last == TRUE), n_false - (s_last == FALSE)
            st.num_solution += n_true
            st.num_failed_node += n_false
            if n_true and len(st.solutions) < keep_solutions:
                rows = torch.nonzero(status == TRUE).flatten()
                if s_last == TRUE:
                    rows = rows[rows != 0]  # (not counted: not kept either)
                rows = rows[: keep_solutions - len(st.solutions)]
                st.solutions += list(kind.unpacked(self.lb[lo:top][rows], stream).cpu().numpy())
                if keep_bounds:
                    if self.ub is None or self.set_words:
                        raise ValueError("keep_bounds needs int32 (lb, ub) rows of an interval store")
                    self.solutions_ub += list(self.ub[lo:top][rows].cpu().numpy())
                if keep_bits:
                    if self.bits is None:
                        raise ValueError("keep_bits needs the sets of a set-mode store")
                    self.solutions_bits += list(self.bits[lo:top][rows].cpu().numpy().view(np.uint64))
            # pop the parents; the children, already in left-first order (branch_reverse), become the new top segment
            self.segs[-1][1] = length - n
            kind.pop(buf, length == n)
            if length == n:
                self.segs.pop()
            if n_true and not all_solutions:
                done = True
                break
            if n_children:
                self.segs.append([top, n_children])
                kind.push(buf)
            st.max_open = max(st.max_open, self.size)
        ctx.set_option("branch_reverse", 0)
        if bnb and st.best is not None:
            st.best_solution = self.best_lb.cpu().numpy().copy()
        s = ctx.stats_read(stream)
        st.filter_steps = s["steps"] + s["steps3"]
        st.evaluated = s.get("evaluated", 0)
        return done or not self.segs

    def run(self, lb0, ub0, all_solutions: bool = True, node_limit: int = 0, keep_solutions: int = 0, base: int = 0) -> DeviceSearchStats:
        self.reset(lb0, ub0, base)
        self.advance(all_solutions=all_solutions, node_limit=node_limit, keep_solutions=keep_solutions)
        return self.stats

    def top(self, k: int):
        """The k open nodes on top of the stack (device tensors, views)."""
        if self.segs and self.segs[-1][1] < min(k, self.size):
            self.compact()
        s, l = self.segs[-1] if self.segs else (0, 0)
        lo = max(s, s + l - k)
        return self.lb[lo:s + l], _cut(self.ub, lo, s + l), _cut(self.act, lo, s + l)
