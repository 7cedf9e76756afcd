"""Device-resident search over FDSpace (IntervalSet<i32> domains) as a FOREST: the batched device search (search_device.DeviceSearch:
pcp_propagate_device + pcp_branch_device_set, 133 KB rows per node) only expands the root breadth-first until there are enough open
nodes; every open node then becomes the root of a tree that ONE workgroup searches depth-first with its current node in LDS and an
undo trail in HBM (pcp_dfs_forest_device_set) — what the reference's VStoreTrail does (variable/memory/trail_memory.rs:100-104),
once per CU.  The union of the expansion and the trees is exactly the reference's search tree (tests/test_set_forest.py).

Several ranks: every rank runs the same expansion (no communication) and takes the open nodes r, r + world, ...; counters are summed
by the caller (one all_reduce).  Between launches a finished tree takes the oldest open node of the tree with the most open nodes —
of its own GPU first, and (interval forest, with a process group) of another rank when its whole GPU ran dry: run_forest_loop /
refill_across_ranks."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from .engine import (FOREST_ENTRIES, FOREST_KINDS, VAR_SELECTS, _check_brancher, _check_collect, _check_enum_forest, _check_forest_brancher, _check_steal,
                     _neq_enum_forest, _xneq_forest, scoped_var_select, store_forest_kind, var_select_scope)


def share_of_budget(node_limit: int, seeded_nodes: int, rank: int, world: int) -> int:
    """This rank's part of what is left of `node_limit` after the expansion: the shares differ by at most one and add up exactly."""
    left = max(int(node_limit) - int(seeded_nodes), 0)
    return left // world + (1 if rank < left % world else 0)


def seed_roots(ctx, lb0, ub0, base: int, want: int, brancher: str = "split", val: str = "middle", collect_solutions: bool = False):
    """Breadth-first expansion of the root to at least `want` open nodes (or until the tree is exhausted) under the distributor
    ``brancher`` ("split": BinarySplit on MiddleVal; "enumerate": Enumerate on ``val``, "middle" or "min").
    Returns (roots [k, V, set_words] int64 CUDA tensor, stats of the expansion).
    ``collect_solutions``: a third value is returned, the solutions the expansion found as products of sets: [n, V, set_words] uint64 numpy
    (the stats' ``solutions`` hold the lower bounds only)."""
    from .search_device import DeviceSearch
    ds = DeviceSearch(ctx, batch=max(want, 1), capacity=4 * max(want, 1) + 64, implicit=True, brancher=brancher, val=val)
    ds.reset(lb0, ub0, base)
    while 0 < ds.size < want:
        if collect_solutions:
            if ds.advance(all_solutions=True, max_rounds=1, keep_solutions=1 << 62, keep_bits=True):
                break
        elif ds.advance(all_solutions=True, max_rounds=1, keep_solutions=0):
            break
    ds.compact()
    k = ds.size
    roots = ds.bits[:k].clone()
    st = ds.stats
    if collect_solutions:
        shape = (int(ds.bits.shape[1]), int(ds.bits.shape[2]))
        return roots, st, (np.stack(ds.solutions_bits).reshape((-1,) + shape) if ds.solutions_bits else np.zeros((0,) + shape, np.uint64))
    return roots, st


def trail_bound(ctx) -> int:
    """The most entries a tree's undo trail can hold: one per value of the root's sets (see forest_search_set)."""
    return int(ctx.n_vars) * int(ctx.set_words) * 64 + 16


@scoped_var_select()
def forest_search_set(ctx, lb0, ub0, base: int = 0, node_limit: int = 0, n_trees: int = 512, steps_per_launch: int = 2048, rank: int = 0, world: int = 1,
                      trail_capacity: int = 0, level_capacity: int = 0, info: dict | None = None, brancher: str = "split", val: str = "middle",
                      formulas: bool = False, rebalance: bool = True, collect_solutions: bool = False, sink_capacity: int = 4096) -> dict:
    """All solutions of the space below (lb0, ub0) — or the first `node_limit` nodes of this rank's share of it.
    brancher / val: the distributor of the expansion AND of the trees ("enumerate": Enumerate on MiddleVal or MinVal), so that their union is
    one tree of that distributor.
    formulas: the store holds formula propagators (Boolean / formula units): the trees run in Context.dfs_forest_setform, one per wavefront,
    instead of dfs_forest_set (the expansion runs such stores as it is).
    trail_capacity / level_capacity 0 = derived from the model (trail_bound): every trail entry takes at least one value out of one
    set and is popped before that value can come back, so a tree's trail never holds more entries than the root has values —
    n_vars * set_words * 64 at most.  (N-queens-1000: 1 024 000 entries = 16 MB per tree; a 100-variable model: 100 KB.)
    rebalance: between launches finished trees take work from the others (pcp_dfs_forest_split_set).
    Returns dict(nodes, solutions, failed, error, seeded_nodes, trees, launches, finished_trees, splits); with world > 1 the expansion's counters are
    reported by rank 0 only, so that a sum over the ranks counts every node once.
    collect_solutions / sink_capacity (one rank; ``world`` > 1 is a ValueError): as for Context.dfs_forest_set — the result also holds
    ``solutions_bits`` ([n, n_vars, set_words] uint64, every solution as a product of sets) and ``solution_tree`` ([n]; -1: a solution the
    expansion found, they come first), and ``seeded_solutions`` counts those."""
    if collect_solutions:
        from .engine import _check_collect_set
        _check_collect_set("forest_search_set", collect_solutions, sink_capacity)
        if world > 1:
            raise ValueError("forest_search_set: collect_solutions does not run on several ranks (gathering the sinks is not built)")
    roots, st, *found = seed_roots(ctx, lb0, ub0, base, n_trees * world, brancher=brancher, val=val, **(dict(collect_solutions=True) if collect_solutions else {}))
    mine = roots[rank::world].contiguous()
    out = {"seeded_nodes": st.num_nodes if rank == 0 else 0, "trees": int(mine.shape[0]), "launches": 0,
           "nodes": st.num_nodes if rank == 0 else 0, "solutions": st.num_solution if rank == 0 else 0, "failed": st.num_failed_node if rank == 0 else 0,
           "error": 0, "finished_trees": 0, "splits": 0}
    if collect_solutions:
        out["solutions_bits"], out["solution_tree"], out["seeded_solutions"] = found[0], np.full(len(found[0]), -1, np.int32), len(found[0])
    budget = 0
    if node_limit:
        budget = share_of_budget(node_limit, st.num_nodes, rank, world)
        if budget == 0:
            return out
    if mine.shape[0] == 0:
        return out
    bound = trail_bound(ctx)
    run = ctx.dfs_forest_setform if formulas else ctx.dfs_forest_set
    r = run(mine, node_limit=budget, steps_per_launch=steps_per_launch, trail_capacity=trail_capacity or bound, level_capacity=level_capacity or min(bound, 1 << 14),
            want_solution=False, info=info, brancher=brancher, val=val, rebalance=rebalance,
            **(dict(collect_solutions=True, sink_capacity=sink_capacity) if collect_solutions else {}))
    out["nodes"] += r["nodes"]; out["solutions"] += r["solutions"]; out["failed"] += r["failed"]
    out["error"] = r["error"]; out["launches"] = r["launches"]; out["finished_trees"] = r["finished_trees"]; out["splits"] = r["splits"]
    if collect_solutions:
        for k in ("solutions_bits", "solution_tree"):
            out[k] = np.concatenate([out[k], r[k]])
    return out


@scoped_var_select()
def forest_bnb_set(ctx, lb0, ub0, base: int, objective, n_trees: int = 256, ramp_steps: int = 16, steps_per_launch: int = 2048, brancher: str = "split",
                   val: str = "middle", best0=None, node_limit: int = 0, trail_capacity: int = 0, level_capacity: int = 0, info: dict | None = None,
                   formulas: bool = False) -> dict:
    """Branch and bound over FDSpace in the forest (branch_and_bound.rs:64-84 around the loop of forest_search_set): minimize / maximize
    ``objective`` = (var, "min" | "max") below (lb0, ub0).  There is no expansion by DeviceSearch: the single root goes to tree 0, the
    other trees start idle, and the incumbent is ONE device word from the root to the end (pcp_dfs_forest_device_set_bnb), so both
    distributors work.  While trees are idle the launches are short (``ramp_steps`` nodes each) and the splits between them hand the
    oldest open right branches to the idle trees; after that the launches are ``steps_per_launch`` nodes.
    formulas: the store holds formula propagators: Context.dfs_forest_setform_bnb instead of dfs_forest_set_bnb.
    Returns the dict of Context.dfs_forest_set_bnb: counters, ``best``, ``best_solution``, ``tree_best``."""
    from .model import interval_bits
    V, sw = int(ctx.n_vars), int(ctx.set_words)
    roots = np.zeros((int(n_trees), V, sw), np.uint64)
    roots[0] = interval_bits(np.asarray(lb0), np.asarray(ub0), sw, base)
    live = np.zeros(int(n_trees), bool)
    live[0] = True
    bound = trail_bound(ctx)
    run = ctx.dfs_forest_setform_bnb if formulas else ctx.dfs_forest_set_bnb
    return run(roots, objective, live=live, best0=best0, brancher=brancher, val=val, steps_per_launch=steps_per_launch, node_limit=node_limit,
               trail_capacity=trail_capacity or bound, level_capacity=level_capacity or min(bound, 1 << 14), info=info,
               ramp_steps=ramp_steps if n_trees > 1 else 0)


def plan_refill(idle, donors):
    """Who sends how many open nodes to whom: ``idle[r]`` trees of rank r have nothing left, ``donors[r]`` trees of rank r have two or
    more open nodes (each can give one).  Only a rank without idle trees gives (one with both fixes itself locally first).  The plan is a
    pure function of the two gathered lists, so every rank computes the same one.  Returns [(src, dst, k)], k >= 1."""
    give = [(r, int(d)) for r, d in enumerate(donors) if d > 0 and idle[r] == 0]
    moves, gi = [], 0
    for dst, need in enumerate(idle):
        need = int(need)
        while need > 0 and gi < len(give):
            src, have = give[gi]
            k = min(need, have)
            moves.append((src, dst, k))
            need -= k
            if have == k:
                gi += 1
            else:
                give[gi] = (src, have - k)
    return moves


def refill_across_ranks(fs, spc, dist, info: dict | None = None) -> int:
    """One exchange of the interval forest: ranks whose trees ran dry receive open nodes from ranks that have trees with two or more.
    ``fs``: this rank's ForestStacks (device or CPU tensors; BinarySplit: ``lb``, ``ub`` and the rows' ``dirty`` hints travel, exclusion
    lists do not), ``spc``: its stack sizes as a numpy array (updated in place).  A donor tree gives its BOTTOM row (its oldest open node:
    the subtree nearest its root), richest trees first; a receiving tree starts from that row.  ONE all_gather of two integers per rank,
    then pairwise send/recv of the rows (RCCL over xGMI with backend nccl; gloo in the tests).  Returns rows sent (+) or received (-)."""
    import torch
    world, rank = dist.get_world_size(), dist.get_rank()
    sp, moving = fs.sp, [t for t in (fs.lb, fs.ub, fs.dirty) if t is not None]
    dev = sp.device
    idle_t = np.nonzero(spc == 0)[0]
    donor_t = [int(i) for i in np.argsort(-spc, kind="stable") if spc[i] >= 2]
    mine = torch.tensor([len(idle_t), len(donor_t)], dtype=torch.int64, device=dev)
    gathered = [torch.zeros(2, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(gathered, mine)
    g = torch.stack(gathered).cpu().numpy()
    moves = plan_refill(g[:, 0].tolist(), g[:, 1].tolist())
    if not moves:
        return 0
    ops, incoming, delta, gave, took = [], [], 0, 0, 0
    for src, dst, k in moves:
        if rank == src:
            trees = donor_t[gave:gave + k]
            gave += k
            idx = torch.tensor(trees, dtype=torch.int64, device=dev)
            ops += [dist.P2POp(dist.isend, t[idx, 0].contiguous(), dst) for t in moving]
            for d in trees:
                fs.drop_bottom(d, int(spc[d]))
                spc[d] -= 1
            sp[idx] -= 1
            delta += k
        elif rank == dst:
            bufs = [torch.empty((k,) + tuple(t.shape[2:]), dtype=t.dtype, device=dev) for t in moving]
            ops += [dist.P2POp(dist.irecv, b, src) for b in bufs]
            incoming.append((bufs, idle_t[took:took + k]))
            took += k
            delta -= k
    if ops:
        for req in dist.batch_isend_irecv(ops):
            req.wait()
    for bufs, trees in incoming:
        idx = torch.tensor(np.asarray(trees), dtype=torch.int64, device=dev)
        for t, b in zip(moving, bufs):
            t[idx, 0] = b
        sp[idx] = 1
        spc[trees] = 1
    if info is not None:
        info["moved_rows"] = info.get("moved_rows", 0) + max(delta, 0)
        info["moved_bytes"] = info.get("moved_bytes", 0) + max(delta, 0) * int(fs.lb.shape[2]) * 8
    return delta


class ForestStacks:
    """The interval forest's state: stacks ``lb``/``ub`` [T, capacity, V], ``status`` [T, capacity], sizes ``sp`` [T], flags ``stop`` [T],
    ``counters`` [T, 5] (nodes, solutions, failed, error, ..).  ``grow()`` doubles the rows per tree (a tree's rows stay where they are
    within its slice) up to ``max_capacity``; ``on_grow`` lets the owner re-point its pcp_dfs_state.
    Under Enumerate (pcp_dfs_forest_device_small_enum) also ``path`` [T, path_capacity, 2] — each tree's exclusions along its current path —
    and per stack row ``row_base`` [T, capacity] and ``row_excl`` [T, capacity, 2] (pcp_forest_excl); ``grow()`` carries the two row arrays,
    ``grow_path()`` doubles the path up to ``max_path``.  ``steal_bottom()`` / ``drop_bottom()`` move a tree's oldest open node."""

    # The per-row arrays (any but lb / ub may be None): name -> (dtype, shape behind [T, capacity] — "V": the variables —, what a fresh row
    # holds (None: it is written before it is read), whether a row takes the word along when it moves to another tree).  dirty: -1 = no hint.
    ROWS = {"lb": ("int32", ("V",), None, True), "ub": ("int32", ("V",), None, True), "status": ("uint8", (), 0, False), "dirty": ("int32", (), -1, True),
            "row_base": ("int32", (), 0, True), "row_excl": ("int32", (2,), 0, True)}

    @classmethod
    def rows(cls, name: str, T: int, capacity: int, V: int, device, dtype=None):
        """A fresh per-row array ``name`` of ``capacity`` rows for each of ``T`` trees."""
        import torch
        kind, tail, fill, _ = cls.ROWS[name]
        dtype = dtype or getattr(torch, kind)
        shape = (T, capacity) + tuple(V if n == "V" else n for n in tail)
        t = torch.empty(shape, dtype=dtype, device=device) if fill is None else torch.full(shape, fill, dtype=dtype, device=device)
        if name == "row_excl":
            t[:, :, 0] = -1  # var 0xFFFFFFFF: the row appends nothing
        return t

    def __init__(self, lb, ub, status, sp, stop, counters, max_capacity: int = 0, on_grow=None, dirty=None, path=None, row_base=None, row_excl=None,
                 path_capacity: int = 0, max_path: int = 0):
        self.lb, self.ub, self.status, self.sp, self.stop, self.counters = lb, ub, status, sp, stop, counters
        self.path, self.row_base, self.row_excl = path, row_base, row_excl
        self.path_capacity = int(path_capacity)  # what the kernel is told (the buffer holds at least one entry)
        self.max_path = int(max_path) if max_path else self.path_capacity
        self.path_grown = 0
        self.dirty = dirty  # moves with its row
        self.max_capacity = int(max_capacity) if max_capacity else int(lb.shape[1])
        self.on_grow = on_grow
        self.grown = 0

    @property
    def capacity(self) -> int:
        return int(self.lb.shape[1])

    def _rows_present(self, moving_only=False) -> list:  # the names of the row arrays this forest has (of those a moving row takes along)
        return [n for n, spec in self.ROWS.items() if getattr(self, n) is not None and (spec[3] or not moving_only)]

    def grow(self) -> bool:
        cap = self.capacity
        new = min(2 * cap, self.max_capacity)
        if new <= cap:
            return False
        T, _, V = self.lb.shape
        for name in self._rows_present():  # (by name: each old array is released before the next new one is allocated)
            old = getattr(self, name)
            t = self.rows(name, T, new, V, old.device, old.dtype)
            t[:, :cap] = old
            setattr(self, name, t)
            del old
        self.grown += 1
        if self.on_grow:
            self.on_grow(self)
        return True

    def grow_path(self) -> bool:
        """Double every tree's exclusion path (entries stay where they are) up to ``max_path``; False at the ceiling."""
        import torch
        cap = self.path_capacity
        new = min(max(2 * cap, 1), self.max_path)
        if new <= cap:
            return False
        t = torch.zeros((self.path.shape[0], new, 2), dtype=self.path.dtype, device=self.path.device)
        t[:, :self.path.shape[1]] = self.path
        self.path, self.path_capacity = t, new
        self.path_grown += 1
        if self.on_grow:
            self.on_grow(self)
        return True

    def drop_bottom(self, d: int, k: int, r=None):
        """Tree ``d`` of ``k`` rows gives its bottom row away — to row 0 of tree ``r`` of this forest, if given — and its stack moves down by
        one row, every word of a row with it.  (``sp`` is the caller's.)"""
        for t in [getattr(self, n) for n in self._rows_present(moving_only=True)]:
            if r is not None:
                t[r, 0] = t[d, 0]
            t[d, 0:k - 1] = t[d, 1:k].clone()

    def steal_bottom(self, d: int, r: int, k: int, prefix: int = 0):
        """The bottom row of tree ``d`` (``k`` >= 2 rows: its oldest open node, the subtree nearest its root) becomes row 0 of the idle tree
        ``r``, and ``d``'s stack moves down.  Under Enumerate the row's list goes along: the first ``prefix`` = row_base[d, 0] entries of
        ``d``'s path are copied (``d`` keeps them — its other rows still use that prefix), the row's own two words move with the row."""
        if self.path is not None:
            self.path[r, :prefix] = self.path[d, :prefix]
        self.drop_bottom(d, k, r)
        self.sp[d] = k - 1
        self.sp[r] = 1


def plan_steal_pairs(sp, n_pairs: int):
    """The (donor, receiver) pairs of one steal round of the Interval forests, planned where ``sp`` lives: torch operations only, no copy to
    the host.  ``sp``: [T] stack sizes.  Donors in the order of a stable sort of -sp (richest first, ties by index), receivers in the order of
    a stable sort of sp != 0 (idle trees first, by index); pair i is (donor_order[i], receiver_order[i]).  Returns an int32 [n_pairs, 2]
    tensor (``n_pairs`` <= T).  Where pair i is valid for pcp_dfs_forest_steal — its donor has two or more rows, its receiver none — it is
    the i-th pair run_forest_loop's host steal forms from its two lists; the valid pairs are a prefix, and the entry drops the rest.  T minus
    the number of live trees is an upper bound on the idle ones and so a sufficient ``n_pairs``."""
    import torch
    T, n = int(sp.shape[0]), int(n_pairs)
    if not 0 <= n <= T:
        raise ValueError(f"plan_steal_pairs: n_pairs must be between 0 and the number of trees ({T}), not {n_pairs}")
    size = sp.to(torch.int64)
    donors = torch.argsort(-size, stable=True)[:n]
    receivers = torch.argsort((size != 0).to(torch.int8), stable=True)[:n]
    return torch.stack([donors, receivers], dim=1).to(torch.int32)


def run_forest_loop(launch, fs: ForestStacks, stop_on_solution: bool = False, node_budget: int = 0, rebalance: bool = True,
                    max_launches: int = 1 << 30, dist=None, sink=None, steal: str = "host", stealer=None) -> dict:
    """The host side of the interval forest (engine.Context._run_row_forest): ``launch()`` enqueues one launch of the forest kernel on the
    stacks ``fs``; between launches a tree whose stack is full gets more rows (ForestStacks.grow: memory follows the depth actually
    reached instead of being reserved for the worst case) and finished trees take work — from trees of this GPU, then (``dist``) from
    other ranks.  With ``dist`` every rank runs the same number of launches and the end of the search / node_budget are decided on
    the all-reduced summary.  Returns dict(launches, steals, moved_rows, moved_bytes, exchange_s, grown, capacity).
    Under Enumerate (``fs.path`` is there; one rank) a tree that reports error 5 gets a longer path (ForestStacks.grow_path) and is resumed
    as one with error 1 is, and a stolen bottom row takes its list along (ForestStacks.steal_bottom).  The result then also names
    ``first_steal``: the donor's bottom node before the first steal and the receiver's row 0 after it, each as (lb, ub, entries [k, 2]).
    ``sink`` (an engine.SolutionSink the entry writes into; one rank): a tree that reports error 6 found the sink full and kept
    its node, propagated and uncounted; the sink is drained, the error and ``stop`` of those trees are cleared, and they resume as trees with
    error 1 do — counters are what a sink that never fills leaves.  The result then also names ``drains``, the drains a full sink forced.
    ``steal``: "host" — the loop below over a host copy of ``sp`` — or "device" (one rank): one plan_steal_pairs and one
    ``stealer(pairs, done)`` call per launch, the caller's pcp_dfs_forest_steal on the forest's CURRENT state (engine.Context.forest_steal).
    Both leave the same state.  The device path copies nothing to the host beyond the launch's summary — the steals are added up on the
    device and read once behind the last launch — except that, until the first steal has happened, ``first_steal`` reads three words back."""
    import time
    import torch
    if steal not in ("host", "device"):
        raise ValueError(f"run_forest_loop: steal must be 'host' or 'device', not {steal!r}")
    T = int(fs.sp.shape[0])
    launches = steals = fatal = drains = 0
    enum = fs.path is not None
    first_steal = stolen = None  # (stolen — steal="device": the steals so far, one device word)
    if steal == "device":
        if dist is not None and dist.get_world_size() > 1:
            raise ValueError("run_forest_loop: steal='device' runs on one rank (refill_across_ranks works from the host's copy of sp)")
        if stealer is None:
            raise ValueError("run_forest_loop: steal='device' needs a stealer (engine.Context.forest_steal on the forest's state)")

    def first_valid(pairs):  # steal="device": (any, donor, receiver) of the first pair the entry will carry out, and the donor's bottom node — all on the device
        d, r = pairs[:, 0].long(), pairs[:, 1].long()
        size = fs.sp.long()
        ok = (d != r) & (size[r] == 0) & (size[d] >= 2) & (size[d] <= fs.capacity) & (fs.row_base[:, 0].long()[d] <= fs.path_capacity)
        i = ok.to(torch.int8).argmax().reshape(1)  # (the first of several maxima; 0 when no pair is valid: still a tree of the forest)
        dd = d[i]
        rows = [t[:, 0].index_select(0, dd)[0] for t in (fs.lb, fs.ub, fs.row_base, fs.row_excl)]
        return torch.cat([ok.any().long().reshape(1), dd, r[i]]), rows + [fs.path.index_select(0, dd)[0]]

    def node(lb, ub, nb, own, path):  # a row as (lb, ub, its list): the path's first nb entries and, if it appends one, the row's own
        own, ent = own.cpu().numpy(), path[:int(nb)].cpu().numpy()
        return lb.cpu().numpy(), ub.cpu().numpy(), (np.concatenate([ent, own[None]]) if own[0] != -1 else ent)

    node_of = lambda t: node(fs.lb[t, 0], fs.ub[t, 0], fs.row_base[t, 0], fs.row_excl[t, 0], fs.path[t])  # row 0 of tree t

    def resume(kept):  # the trees of the mask kept their node on top of the stack, uncounted: clear their error and ``stop``
        idx = torch.nonzero(kept).flatten()
        fs.counters[idx, 3] = 0
        fs.stop[idx] = 0

    xinfo, exchange_s = {"moved_rows": 0, "moved_bytes": 0}, 0.0
    multi = dist is not None and dist.get_world_size() > 1
    zero = torch.zeros((), dtype=torch.int64, device=fs.sp.device)
    while launches < max_launches:
        launch()
        launches += 1
        sp, stop, counters = fs.sp, fs.stop, fs.counters
        live = (sp > 0) & (stop == 0)
        err = counters[:, 3]
        # errors that hand a node back (pcp_hip.h, pcp_dfs_device: it stayed on top of its stack, uncounted): 1 — the stack is full; 5 — the
        # exclusion path is full (Enumerate); 6 — the solution sink is full.  Anything else ends the search.
        full = handed = err == 1
        pfull = sfull = None
        if enum:
            pfull = err == 5
            handed = handed | pfull
        if sink is not None:
            sfull = err == 6
            handed = handed | sfull
        # one summary of one shape (zeros where a feature is off), so that every rank reduces the same words
        summary = torch.stack([live.sum(), counters[:, 0].sum(), counters[:, 1].sum(), full.sum(), ((err != 0) & ~handed).sum() + fatal,
                               pfull.sum() if enum else zero, sfull.sum() if sink is not None else zero]).to(torch.int64)
        mine = summary.cpu().tolist()  # (the launch's only synchronisation on one GPU)
        vals = mine
        if multi:
            t0 = time.perf_counter()
            dist.all_reduce(summary, op=dist.ReduceOp.SUM)
            vals = summary.cpu().tolist()
            exchange_s += time.perf_counter() - t0
        if vals[4] or (stop_on_solution and vals[2]) or (node_budget and vals[1] >= node_budget):
            break
        if mine[3]:
            if fs.grow():
                resume(full)
            elif not multi:
                break  # the ceiling is reached: the trees keep error 1 (the caller reports it)
            else:
                fatal = 1  # (several ranks leave the loop TOGETHER: the flag travels with the next launch's summary)
        elif not (mine[5] or mine[6]) and vals[0] == 0 and vals[3] == 0:
            break
        if mine[5]:
            if not fs.grow_path():
                break  # the ceiling is reached: the trees keep error 5
            resume(pfull)
        if mine[6]:
            sink.drain()
            drains += 1
            resume(sfull)
        if not rebalance:
            continue
        sp = fs.sp
        spc = None
        if mine[0] < T and steal == "device":
            # The same steals, planned and carried out on the device: T - live is an upper bound on the idle trees, the entry drops every
            # pair that is not (a tree with two or more rows, an idle tree).
            pairs = plan_steal_pairs(sp, T - mine[0])
            done = torch.empty(pairs.shape[0], dtype=torch.int32, device=sp.device)
            watch = first_valid(pairs) if enum and first_steal is None else None
            stealer(pairs, done)
            stolen = done.sum() if stolen is None else stolen + done.sum()
            if watch is not None:
                some, d, r = watch[0].cpu().tolist()
                if some:
                    first_steal = {"donor": d, "receiver": r, "before": node(*watch[1]), "after": node_of(r)}
        elif mine[0] < T:
            # Finished trees take work from the others (ForestStacks.steal_bottom).  Counters stay per tree, so their sum is the search's.
            # (With a per-tree node limit a tree that reached it must stay stopped.)
            spc = sp.cpu().numpy().copy()
            idle = [int(i) for i in np.nonzero(spc == 0)[0]]
            donors = [int(i) for i in np.argsort(-spc, kind="stable") if spc[i] >= 2][:len(idle)]
            rb0 = fs.row_base[:, 0].cpu().numpy() if enum and donors else None
            for d, r in zip(donors, idle):
                before = node_of(d) if enum and first_steal is None else None
                fs.steal_bottom(d, r, int(spc[d]), int(rb0[d]) if enum else 0)
                spc[d] -= 1; spc[r] = 1
                steals += 1
                if before is not None:
                    first_steal = {"donor": d, "receiver": r, "before": before, "after": node_of(r)}
        if multi:
            t0 = time.perf_counter()
            if spc is None:
                spc = sp.cpu().numpy().copy()
            refill_across_ranks(fs, spc, dist, xinfo)
            exchange_s += time.perf_counter() - t0
    if stolen is not None:
        steals += int(stolen.item())
    out = {"launches": launches, "steals": steals, "moved_rows": xinfo["moved_rows"], "moved_bytes": xinfo["moved_bytes"], "exchange_s": exchange_s,
           "grown": fs.grown, "capacity": fs.capacity}
    if enum:
        out["first_steal"] = first_steal
    if sink is not None:
        out["drains"] = drains
    return out


# What a breadth-first expansion left (_seed_interval): the open nodes' rows, the expansion's stats, each root's exclusion list (a [k, 2] int32
# array of (var, value); None under BinarySplit) and the solutions it found as boxes ((lb rows, ub rows); None unless asked for).
Seeds = namedtuple("Seeds", "lb ub stats lists boxes")


def _seed_interval(ctx, lb0, ub0, want: int, objective=None, brancher: str = "split", val: str = "middle", collect_solutions: bool = False) -> Seeds:
    from .search_device import DeviceSearch
    ds = DeviceSearch(ctx, batch=max(want, 1), capacity=4 * max(want, 1) + 64, implicit=True, objective=objective, brancher=brancher, val=val)
    ds.reset(lb0, ub0)
    while 0 < ds.size < want:
        if collect_solutions:
            if ds.advance(all_solutions=True, max_rounds=1, keep_solutions=1 << 62, keep_bounds=True):
                break
        elif ds.advance(all_solutions=True, max_rounds=1, keep_solutions=0):
            break
    ds.compact()
    k = ds.size
    lists = boxes = None
    if collect_solutions:
        V = int(ds.lb.shape[1])
        rows = lambda r: np.stack(r).astype(np.int32).reshape(-1, V) if r else np.zeros((0, V), np.int32)
        boxes = (rows(ds.stats.solutions), rows(ds.solutions_ub))
    if brancher != "split":
        lists = []
        if k:  # the one segment's offsets (relative to its first entry) and entries
            o, e0, _, _ = ds.esegs[-1]
            off = ds.eoff[o:o + k + 1].cpu().numpy().astype(np.int64)
            ex = ds.ex[e0:e0 + int(off[-1])].cpu().numpy().reshape(-1, 2)
            lists = [np.ascontiguousarray(ex[off[i]:off[i + 1]], np.int32) for i in range(k)]
    return Seeds(ds.lb[:k].clone(), ds.ub[:k].clone(), ds.stats, lists, boxes)


def seed_roots_interval(ctx, lb0, ub0, want: int, objective=None, brancher: str = "split", val: str = "middle", collect_solutions: bool = False):
    """Interval mode: breadth-first expansion of the root to at least `want` open nodes.  ``objective``: the expansion runs under branch and
    bound (DeviceSearch(objective=)), its stats carry the incumbent (``best``, ``best_solution``).  Returns (lb rows, ub rows, stats).
    ``brancher="enumerate"``: the expansion runs under Enumerate on ``val`` (DeviceSearch(brancher="enumerate", val=, objective=)) and a
    fourth value is returned: each root's exclusion list, a [k, 2] int32 array of (var, value).
    ``collect_solutions``: one more value is returned behind the others, the solutions the expansion found as boxes: (lb rows, ub rows),
    two [n, V] int32 numpy arrays (the stats' ``solutions`` hold the lower bounds only)."""
    s = _seed_interval(ctx, lb0, ub0, want, objective=objective, brancher=brancher, val=val, collect_solutions=collect_solutions)
    return (s.lb, s.ub, s.stats) + (() if s.lists is None else (s.lists,)) + (() if s.boxes is None else (s.boxes,))


STACK_BYTES_CAP = 64 << 30  # default ceiling of the forest's stack rows per GPU (both bound arrays together); rows are allocated as trees get deep


def _expand_and_search(ctx, lb0, ub0, kind: str, brancher: str, val: str, n_trees: int, objective=None, best0=None, collect: bool = False, sink_capacity: int = 4096,
                       capacity: int = 0, max_capacity=None, node_limit: int = 0, rank: int = 0, world: int = 1, dist=None, stack_bytes: int = STACK_BYTES_CAP, **run) -> dict:
    """What forest_search, forest_bnb, forest_enumerate and forest_solutions share: expand the root breadth-first under the distributor
    (_seed_interval), run this rank's open nodes as the trees of the forest ``kind`` ("neq" | "small" | "form"), and merge — the
    expansion's counters are added to the trees', its solutions come first (``solution_tree`` -1), its incumbent is the forest's first.
    The Context method follows from kind, brancher and objective: dfs_forest_enum under Enumerate, dfs_forest_bnb under BinarySplit with an
    objective, dfs_forest_neq_solutions for the all-XNeqY forest's solutions, else dfs_forest; ``run``: further keywords for it (steps_per_launch,
    info, steal, ..).  ``max_capacity`` None: the stacks are sized from ``node_limit`` and ``stack_bytes``, as forest_search describes."""
    enum = brancher == "enumerate"
    s = _seed_interval(ctx, lb0, ub0, n_trees * world, objective=objective, brancher=brancher, val=val, collect_solutions=collect)
    st = s.stats
    ml, mu = s.lb[rank::world].contiguous(), s.ub[rank::world].contiguous()
    first = rank == 0  # (with world > 1 the expansion's counters are reported by rank 0 only: a sum over the ranks counts every node once)
    out = {"seeded_nodes": st.num_nodes if first else 0, "trees": int(ml.shape[0]), "launches": 0,
           "nodes": st.num_nodes if first else 0, "solutions": st.num_solution if first else 0, "failed": st.num_failed_node if first else 0, "error": 0}
    if collect:
        out.update(solutions_lb=s.boxes[0], solutions_ub=s.boxes[1], solution_tree=np.full(len(s.boxes[0]), -1, np.int32), seeded_solutions=len(s.boxes[0]))
    budget = share_of_budget(node_limit, st.num_nodes, rank, world) if node_limit else 0
    multi = dist is not None and world > 1
    sp0, run_trees = None, True
    if multi:
        # the loop below is collective (an all_reduce and an all_gather per launch): every rank enters it or none does — decided on what is
        # left of the GLOBAL budget, the same number on every rank.  A rank without a share, or without a tree, still takes part: it
        # brings one tree with an empty stack, which the cross-rank refill can hand work to.
        if (node_limit and node_limit - st.num_nodes <= 0) or s.lb.shape[0] == 0:  # (the expansion used the budget up / finished the tree)
            run_trees = False
        elif ml.shape[0] == 0:
            ml, mu = s.lb[:1].clone(), s.ub[:1].clone()
            sp0 = [0]
    elif (node_limit and budget == 0) or ml.shape[0] == 0:
        run_trees = False
    if not run_trees and objective is None:
        return out
    if run_trees:
        per_tree = -(-budget // ml.shape[0]) if budget else 0
        if max_capacity is not None:
            max_capacity = max(max_capacity, capacity)
        else:
            # a tree's stack grows by at most one row per node it explores: never more than its share of the budget; it starts at 128 rows
            # (1 MB per tree and bound array at V = 1000) and is doubled when a tree fills it, up to `stack_bytes` for the whole forest
            ceiling = max(64, int(stack_bytes) // (int(ml.shape[0]) * int(ml.shape[1]) * 8))
            if per_tree and not multi:
                ceiling = min(ceiling, per_tree + 64)
            if not capacity:
                # a KNOWN bound (one rank: a tree never holds more rows than its share of the node budget) is allocated at once when it is at most
                # an eighth of the free HBM — growing to it step by step costs three allocations and two copies of a short search; without a
                # bound (no budget, or several ranks with a global budget and refill) a tree starts at 128 rows and grows on demand
                row_bytes = int(ml.shape[0]) * int(ml.shape[1]) * 8
                upfront = 8 << 30
                if ml.is_cuda:
                    import torch
                    upfront = max(upfront, torch.cuda.mem_get_info(ml.device)[0] // 8)
                capacity = ceiling if (per_tree and not multi and ceiling * row_bytes <= upfront) else min(128, ceiling)
            max_capacity = max(ceiling, capacity)
        run.update(node_limit_per_tree=0 if multi else per_tree, capacity=capacity, max_capacity=max_capacity,
                   node_budget=max(node_limit - st.num_nodes, 1) if multi else budget, dist=dist if multi else None)
    if objective is not None:
        # branch and bound: the expansion's incumbent — or ``best0``, whichever is better — is the forest's first one
        mode = objective[1]
        known = [b for b in (best0, st.best) if b is not None]
        start = (min if mode == "min" else max)(known) if known else None
        if not run_trees:  # the expansion finished the tree
            r = {"nodes": 0, "solutions": 0, "failed": 0, "error": 0, "open": 0, "launches": 0, "trees": 0, "steals": 0, "tree_best": np.zeros(0, np.int32),
                 "best": None, "best_solution": None}
        elif enum:
            r = ctx.dfs_forest_enum(ml, mu, val=val, objective=objective, best0=start, root_excl=s.lists, forest=kind, **run)
        else:
            r = ctx.dfs_forest_bnb(ml, mu, objective, best0=start, small=kind == "small", **run)
        r["seeded_nodes"] = st.num_nodes
        r["nodes"] += st.num_nodes; r["solutions"] += st.num_solution; r["failed"] += st.num_failed_node
        # no tree beat the expansion's incumbent: it is the optimum, unless the caller's bound was already as good
        beats = lambda a, b: b is None or (a < b if mode == "min" else a > b)
        if r["best"] is None and st.best is not None and beats(st.best, best0):
            r["best"], r["best_solution"] = st.best, st.best_solution
        return r
    if enum and not (collect and kind == "neq"):
        r = ctx.dfs_forest_enum(ml, mu, val=val, root_excl=s.lists, forest=kind, collect_solutions=collect, sink_capacity=sink_capacity, **run)
    elif collect and kind == "neq":
        r = ctx.dfs_forest_neq_solutions(ml, mu, brancher=brancher, val=val, root_excl=s.lists, sink_capacity=sink_capacity, **run)
    else:
        r = ctx.dfs_forest(ml, mu, sp0=sp0, formulas=kind == "form", small=kind == "small", collect_solutions=collect, sink_capacity=sink_capacity, **run)
    out["nodes"] += r["nodes"]; out["solutions"] += r["solutions"]; out["failed"] += r["failed"]
    out["error"] = r["error"]; out["launches"] = r["launches"]
    if collect:
        for k in ("solutions_lb", "solutions_ub", "solution_tree"):
            out[k] = np.concatenate([out[k], r[k]])
    return out


@scoped_var_select(refuse=_xneq_forest)
def forest_search(ctx, lb0, ub0, node_limit: int = 0, n_trees: int = 768, steps_per_launch: int = 512, rank: int = 0, world: int = 1, capacity: int = 0,
                  dist=None, info: dict | None = None, stack_bytes: int = STACK_BYTES_CAP, formulas: bool = False, small: bool = False, brancher: str = "split",
                  val: str = "middle", collect_solutions: bool = False, sink_capacity: int = 4096, steal: str = "host") -> dict:
    """Interval mode, all-XNeqY models: expansion + one in-kernel DFS per open node (pcp_dfs_forest_device).  formulas: the store holds
    formula propagators (what Cumulative.join builds): the trees run in pcp_dfs_forest_device_form, one per wavefront.  small: a small store of
    plain propagators of any kind (the Golomb network): pcp_dfs_forest_device_small, one tree per wavefront; with formulas=True a ValueError.  The node limit is checked
    between launches, so `nodes` can exceed it by less than one launch; it is the exact count.  Without ``dist`` every tree also stops at
    its share of the limit; with ``dist`` (torch.distributed, world ranks) the limit is global, finished trees are refilled (also across
    ranks) and the returned counters are still this rank's.  A tree's stack holds its OPEN nodes (one right branch per level of
    its current path); the rows are allocated on demand (ForestStacks.grow) up to ``stack_bytes`` for the whole forest — a tree
    that needs more reports error 1.
    brancher / val: the distributor of the expansion AND of the trees ("enumerate": Enumerate on MiddleVal or MinVal; small=True only, one
    rank — with ``dist``, ``world`` > 1, ``formulas=True`` or the all-XNeqY forest a ValueError): the roots arrive with the exclusion lists the
    expansion gave them, so that the expansion and the trees together are one Enumerate tree.
    collect_solutions / sink_capacity (formulas=True or small=True, one rank; otherwise a ValueError): as for Context.dfs_forest — the result
    also holds ``solutions_lb`` / ``solutions_ub`` ([n, n_vars] int32, every solution as a box) and ``solution_tree`` ([n]; -1: a solution the
    expansion found, they come first), and ``seeded_solutions`` counts those.
    steal: "host" | "device", how finished trees take work between launches — as for Context.dfs_forest, which it is handed to; "device" with
    a ``dist`` of more than one rank, or any other value, is a ValueError before anything runs."""
    _check_steal("forest_search", steal, dist if world > 1 else None)
    if small and formulas:
        raise ValueError("forest_search: small=True and formulas=True name two different forests (a store has formula units or it has none)")
    enum = _check_forest_brancher("forest_search", brancher, val, small, dist)
    if enum and world > 1:
        raise ValueError("forest_search: brancher='enumerate' does not run on several ranks (moving exclusion lists between ranks is not built)")
    _check_collect("forest_search", collect_solutions, sink_capacity, small, formulas, dist if dist is not None else (True if world > 1 else None))
    return _expand_and_search(ctx, lb0, ub0, "small" if small else "form" if formulas else "neq", brancher, val, n_trees, steps_per_launch=steps_per_launch, info=info, steal=steal,
                              collect=collect_solutions, sink_capacity=sink_capacity, capacity=capacity, node_limit=node_limit, rank=rank, world=world, dist=dist,
                              stack_bytes=stack_bytes)


def forest_solutions(ctx, lb0, ub0, brancher: str = "split", val: str = "middle", n_trees: int = 256, forest=None, sink_capacity: int = 4096,
                     steps_per_launch: int = 512, capacity: int = 128, max_capacity: int = 1 << 16, path_capacity: int = 64, rebalance: bool = True,
                     info: dict | None = None, objective=None, var_select=None, dist=None, steal: str = "host") -> dict:
    """AllSolution (search/engine/all_solution.rs) over the context's Interval store: EVERY solution below (lb0, ub0), as boxes, whichever
    forest the store belongs to.  The root is expanded breadth-first under DeviceSearch (``brancher`` "split" | "enumerate" on ``val``
    "middle" | "min") to at least ``n_trees`` open nodes, each becomes a tree of the forest, and the result is forest_search's dict with
    ``solutions_lb`` / ``solutions_ub`` ([n, n_vars] int32), ``solution_tree`` ([n]; -1: a solution the expansion found, they come first)
    and ``seeded_solutions``.
    ``forest`` (None / "neq" / "small" / "form"; anything else a ValueError): None chooses by the store (Context.forest_kind) — "form"
    with formula units, "neq" for an all-XNeqY store beyond the small-store limits, else "small"; a name forces that forest.  "neq" is the
    all-XNeqY in-kernel forest through Context.dfs_forest_neq_solutions (pcp_dfs_forest_device_neq_sink: the sink is an argument of every
    launch, nothing is attached to the context): any all-XNeqY store the in-kernel search takes (N-queens-1000; forced, small N-queens
    too) — on a store that is not all-XNeqY a ValueError; its stacks grow up to ``max_capacity`` rows.  "small" and "form" collect through
    the context's sink, as forest_search(collect_solutions=True) does, with its stack sizing.
    One rank; ``objective``, ``var_select="input_order"`` with the "neq" forest, ``sink_capacity`` < 1 and ``dist`` are a ValueError before
    anything runs.  ``steal``: "host" | "device", as for Context.dfs_forest."""
    who = "forest_solutions"
    _check_steal(who, steal)
    if forest not in FOREST_KINDS:
        raise ValueError(f"{who}: forest must be None, 'neq', 'small' or 'form', not {forest!r}")
    _check_brancher(brancher, val)
    if objective is not None:
        raise ValueError(f"{who}: every solution is returned, none is preferred (forest_bnb / forest_enumerate(objective=) run branch and bound)")
    if dist is not None:
        raise ValueError(f"{who}: collecting solutions does not run on several ranks (gathering the sinks is not built)")
    if int(sink_capacity) < 1:
        raise ValueError(f"{who}: sink_capacity must be at least 1, not {sink_capacity}")
    if var_select is not None and var_select not in VAR_SELECTS:
        raise ValueError(f"{who}: var_select must be 'first_smallest' or 'input_order', not {var_select!r}")
    neq_refusal = f"{who}: var_select='input_order' " + _neq_enum_forest({"forest": "neq"}, FOREST_ENTRIES["neq", "sink"])
    if forest == "neq" and var_select == "input_order":
        raise ValueError(neq_refusal)
    if forest is None:
        forest = store_forest_kind(ctx)
    if forest == "neq" and not ctx.all_neq:
        raise ValueError(f"{who}: forest='neq' is the all-XNeqY in-kernel forest and this store is not all-XNeqY (forest=None chooses by the store)")
    run = dict(path_capacity=path_capacity, rebalance=rebalance) if (forest == "neq" or brancher == "enumerate") else {}
    if forest == "neq":
        run["max_capacity"] = max_capacity
    with var_select_scope(ctx, var_select):
        if forest == "neq" and ctx.var_select == "input_order":
            raise ValueError(neq_refusal)
        return _expand_and_search(ctx, lb0, ub0, forest, brancher, val, n_trees, steps_per_launch=steps_per_launch, info=info, steal=steal, collect=True, sink_capacity=sink_capacity,
                                  capacity=capacity, **run)


@scoped_var_select()
def forest_bnb(ctx, lb0, ub0, objective, n_trees: int = 256, steps_per_launch: int = 512, best0=None, capacity: int = 128, max_capacity: int = 1 << 16,
               info: dict | None = None, formulas: bool = True, small: bool = False, brancher: str = "split", val: str = "middle",
               collect_solutions: bool = False, steal: str = "host") -> dict:
    """Branch and bound over an Interval store with formula propagators (branch_and_bound.rs:64-84 around the loop of forest_search):
    minimize / maximize ``objective`` = (var, "min" | "max") below (lb0, ub0).  The root is expanded breadth-first under branch and bound
    (seed_roots_interval with DeviceSearch(objective=)) to at least ``n_trees`` open nodes; each becomes a tree of
    Context.dfs_forest_bnb, and the expansion's incumbent — or ``best0``, whichever is better — is the forest's first one, so the
    expansion's solutions take part.  Returns the dict of Context.dfs_forest_bnb (``nodes`` / ``solutions`` / ``failed`` include the
    expansion's, ``seeded_nodes`` names them); ``best`` is None when neither the expansion nor a tree found a solution beating ``best0``.
    ``small``: a small store of plain propagators instead (Context.dfs_forest_bnb(small=True) — model.golomb_ruler); it wins over
    ``formulas``, whose default is True.  brancher / val: as for forest_search — Enumerate needs ``small=True``; the expansion then
    runs under DeviceSearch(brancher="enumerate", val=, objective=) and the roots keep their exclusion lists.
    collect_solutions=True is a ValueError: branch and bound returns ``best_solution``.  steal: "host" | "device", as for Context.dfs_forest."""
    _check_steal("forest_bnb", steal)
    if collect_solutions:
        raise ValueError("forest_bnb: collect_solutions does not go with branch and bound (it keeps best_solution; the entries refuse a solution sink)")
    if not formulas and not small:
        raise ValueError("forest_bnb searches stores with formula propagators (all-XNeqY stores have no objective to bound)")
    _check_forest_brancher("forest_bnb", brancher, val, small, None)
    var, mode = objective
    return _expand_and_search(ctx, lb0, ub0, "small" if small else "form", brancher, val, n_trees, steps_per_launch=steps_per_launch, info=info, steal=steal, objective=(int(var), mode), best0=best0,
                              capacity=capacity, max_capacity=max_capacity)


@scoped_var_select(refuse=_neq_enum_forest)
def forest_enumerate(ctx, lb0, ub0, val: str = "middle", objective=None, n_trees: int = 256, steps_per_launch: int = 512, best0=None, collect_solutions: bool = False,
                     sink_capacity: int = 4096, info: dict | None = None, capacity: int = 128, max_capacity: int = 1 << 16, path_capacity: int = 64, rebalance: bool = True,
                     dist=None, forest=None, steal: str = "host") -> dict:
    """Enumerate over the context's Interval store, whichever forest it belongs to: the root is expanded breadth-first under
    DeviceSearch(brancher="enumerate", val=, objective=) to at least ``n_trees`` open nodes, each becomes a tree of Context.dfs_forest_enum
    with the exclusion list the expansion gave it as its ``root_excl``, so that the expansion and the trees together are one Enumerate
    tree.  Without ``objective`` it returns forest_search's dict (``collect_solutions`` / ``sink_capacity``: every solution as a box, the
    expansion's first) and sizes the stacks as forest_search does from ``capacity``; with ``objective`` = (var, "min" | "max") it returns
    forest_bnb's dict (``best0``: a known bound to start from; the stacks grow up to ``max_capacity`` rows).  ``path_capacity``: a tree's
    exclusion path at first.  One rank: ``dist`` is a ValueError, as are a ``val`` other than "middle" / "min" and ``collect_solutions``
    with an objective.  ``forest`` (None / "neq" / "small" / "form"): the keyword, the choice and the refusals of Context.dfs_forest_enum,
    made before the expansion runs.  ``steal``: "host" | "device", as for Context.dfs_forest."""
    _check_steal("forest_enumerate", steal)
    # (the choice of Context.dfs_forest_enum, made here so that the refusals come before the expansion runs)
    forest = _check_enum_forest("forest_enumerate", ctx, forest, dist, val, objective, collect_solutions, "returns best_solution")
    if objective is not None:
        var, mode = objective
        return _expand_and_search(ctx, lb0, ub0, forest, "enumerate", val, n_trees, steps_per_launch=steps_per_launch, info=info, steal=steal, objective=(int(var), mode), best0=best0,
                                  capacity=capacity, max_capacity=max_capacity, path_capacity=path_capacity, rebalance=rebalance)
    _check_collect("forest_search", collect_solutions, sink_capacity, forest == "small", forest == "form", None)
    return _expand_and_search(ctx, lb0, ub0, forest, "enumerate", val, n_trees, steps_per_launch=steps_per_launch, info=info, steal=steal, collect=collect_solutions, sink_capacity=sink_capacity,
                              capacity=capacity, path_capacity=path_capacity, rebalance=rebalance)
