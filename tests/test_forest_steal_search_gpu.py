"""steal="device" against steal="host", end to end: the same roots through the same forest under both.  A steal leaves the same state behind
whoever carries it out, and what a tree does with its rows does not depend on when it runs, so every tree's counters, the number of
launches and the number of steals must agree, and with a sink the multiset of solution boxes.  Few trees and short launches, so that dozens
of steals happen; a run that never steals shows nothing, so steals > 0 is asserted under both settings.

Under branch and bound the trees of one launch share the incumbent while they run, so which nodes a tree prunes depends on when another tree
finds its solution — under either steal, from one run to the next.  There the optimum is compared (and that it is the known one); whether
the per-tree counters happened to agree is printed.

A sink that FILLS is timing of the same kind: which tree draws the ticket beyond the capacity, and so ends its launch early with its node
handed back, is an order in time between the trees of one launch (pcp_hip.h, pcp_solution_sink), so the stacks a steal finds differ from
run to run under either steal.  Measured on one MI355X with the sinks below (2 rows on N-queens 8, 8 rows on Golomb 6): the totals agreed
(748 / 1288 / 17664 nodes) and the launches (46 / 47 / 826), the steals did not — host against device 67 / 75, 100 / 95, 149 / 145, and host
against a second host run 67 / 68, 100 / 104, 149 / 164 — and most trees' counters differed, between two host runs as well.  There the
totals and the multiset of boxes are compared, and a second host run is printed next to the first;
with a sink that never fills every tree's counters must agree as without one."""
import numpy as np
import pytest

import form_forest_cases as FC
import small_forest_cases as SC
from pcp_amd import model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


def push_store(ctx, vs, cs):
    M.push_model(ctx, cs, len(vs))
    lb0, ub0 = vs.bounds()
    return np.ascontiguousarray(lb0, np.int32), np.ascontiguousarray(ub0, np.int32)


def push_queens(ctx, n=8):
    ctx.set_model(n, M.nqueens_props(n))
    return np.ones(n, np.int32), np.full(n, n, np.int32)


def roots_of(ctx, lb0, ub0, trees, val=None):
    """The open nodes of a breadth-first expansion: (lb rows, ub rows, exclusion lists or None)."""
    from pcp_amd.search_forest import seed_roots_interval
    if val is None:
        rl, ru, _ = seed_roots_interval(ctx, lb0, ub0, trees)
        return rl, ru, None
    rl, ru, _, lists = seed_roots_interval(ctx, lb0, ub0, trees, brancher="enumerate", val=val)
    return rl, ru, lists


def boxes(r):
    return sorted(tuple(a.tolist()) + tuple(b.tolist()) for a, b in zip(r["solutions_lb"], r["solutions_ub"]))


def both(run, what, bnb=False, full_sink=False):
    """run(steal, info) under both settings; the comparisons every case shares.  Returns (host result, device result, infos)."""
    out, infos = {}, {}
    for steal in ("host", "device"):
        infos[steal] = {}
        out[steal] = run(steal, infos[steal])
    h, d = out["host"], out["device"]
    same = np.array_equal(h["per_tree"], d["per_tree"])
    print(what, "trees", h["trees"], "launches", h["launches"], d["launches"], "steals", h["steals"], d["steals"], "nodes", h["nodes"], d["nodes"], "per_tree equal", same)
    assert h["error"] == 0 and d["error"] == 0 and h["open"] == 0 and d["open"] == 0, what
    assert h["steals"] > 0 and d["steals"] > 0, (what, h["steals"], d["steals"])
    if full_sink:
        again = run("host", {})
        print(what, "host against host: per_tree equal", np.array_equal(h["per_tree"], again["per_tree"]), "steals", h["steals"], again["steals"])
        assert (h["nodes"], h["solutions"], h["failed"]) == (d["nodes"], d["solutions"], d["failed"]), what
    elif not bnb:
        assert same, (what, np.nonzero((h["per_tree"] != d["per_tree"]).any(axis=1))[0])
        assert h["launches"] == d["launches"] and h["steals"] == d["steals"], what
        assert (h["nodes"], h["solutions"], h["failed"]) == (d["nodes"], d["solutions"], d["failed"])
    if "solutions_lb" in h:
        assert boxes(h) == boxes(d), what
        assert len(h["solutions_lb"]) == h["solutions"]
    return h, d, infos


# ------------------------------------------------------------------------------------------------ N-queens 8, the all-XNeqY forest
@pytest.mark.parametrize("hints", [True, False], ids=["hints", "no_hints"])
def test_queens_binary_split(ctx, hints):
    lb0, ub0 = push_queens(ctx)
    rl, ru, _ = roots_of(ctx, lb0, ub0, 24)
    both(lambda steal, info: ctx.dfs_forest(rl, ru, steps_per_launch=4, capacity=32, hints=hints, steal=steal, info=info), ("queens8 split", hints))


@pytest.mark.parametrize("val", ["middle", "min"])
def test_queens_enumerate_with_a_growing_path(ctx, val):
    lb0, ub0 = push_queens(ctx)
    rl, ru, lists = roots_of(ctx, lb0, ub0, 24, val=val)
    h, d, infos = both(lambda steal, info: ctx.dfs_forest_enum(rl, ru, val=val, root_excl=lists, forest="neq", path_capacity=1, steps_per_launch=4, capacity=32,
                                                              steal=steal, info=info), ("queens8 enumerate", val))
    for steal in ("host", "device"):
        fs = infos[steal]["first_steal"]
        (bl, bu, be), (al, au, ae) = fs["before"], fs["after"]
        assert fs["donor"] != fs["receiver"] and np.array_equal(bl, al) and np.array_equal(bu, au), steal
        assert {tuple(p) for p in be.tolist()} == {tuple(p) for p in ae.tolist()}, steal
    a, b = infos["host"]["first_steal"], infos["device"]["first_steal"]
    assert (a["donor"], a["receiver"]) == (b["donor"], b["receiver"])
    assert all(np.array_equal(x, y) for x, y in zip(a["before"], b["before"]))
    if val == "middle":
        assert infos["host"]["path_grown"] > 0 and infos["device"]["path_grown"] == infos["host"]["path_grown"]


@pytest.mark.parametrize("brancher,val", [("split", "middle"), ("enumerate", "middle")])
def test_queens_every_solution_through_a_two_row_sink(ctx, brancher, val):
    lb0, ub0 = push_queens(ctx)
    rl, ru, lists = roots_of(ctx, lb0, ub0, 24, val=val if brancher == "enumerate" else None)
    kw = dict(brancher="enumerate", val=val, root_excl=lists) if brancher == "enumerate" else {}
    h, d, infos = both(lambda steal, info: ctx.dfs_forest_neq_solutions(rl, ru, sink_capacity=2, steps_per_launch=4, capacity=32, steal=steal, info=info, **kw),
                       ("queens8 sink", brancher), full_sink=True)
    assert infos["host"]["drains"] > 0 and infos["device"]["drains"] > 0
    # a sink that never fills: nothing is handed back, and every tree does the same under both steals
    _, _, infos = both(lambda steal, info: ctx.dfs_forest_neq_solutions(rl, ru, sink_capacity=4096, steps_per_launch=4, capacity=32, steal=steal, info=info, **kw),
                       ("queens8 roomy sink", brancher))
    assert infos["host"]["drains"] == 0 and infos["device"]["drains"] == 0


# ------------------------------------------------------------------------------------------------ Golomb 6, the small-store forest
def golomb_roots(ctx, trees, val=None):
    vs, cs, var = SC.golomb(6)
    lb0, ub0 = push_store(ctx, vs, cs)
    return roots_of(ctx, lb0, ub0, trees, val=val) + (var,)


@pytest.mark.parametrize("brancher", ["split", "enumerate"])
def test_golomb_small_store(ctx, brancher):
    rl, ru, lists, _ = golomb_roots(ctx, 16, val="middle" if brancher == "enumerate" else None)
    kw = dict(brancher="enumerate", val="middle", root_excl=lists) if brancher == "enumerate" else {}
    both(lambda steal, info: ctx.dfs_forest(rl, ru, small=True, steps_per_launch=16, capacity=64, steal=steal, info=info, **kw), ("golomb6", brancher))


@pytest.mark.parametrize("brancher", ["split", "enumerate"])
def test_golomb_branch_and_bound(ctx, brancher):
    rl, ru, lists, var = golomb_roots(ctx, 16, val="middle" if brancher == "enumerate" else None)
    kw = dict(brancher="enumerate", val="middle", root_excl=lists) if brancher == "enumerate" else {}
    h, d, _ = both(lambda steal, info: ctx.dfs_forest_bnb(rl, ru, (var, "min"), small=True, steps_per_launch=16, capacity=64, steal=steal, info=info, **kw),
                   ("golomb6 bnb", brancher), bnb=True)
    assert h["best"] == d["best"] == SC.OPTIMUM[6]
    assert SC.is_ruler(h["best_solution"], 6) and SC.is_ruler(d["best_solution"], 6)


def test_golomb_collect_solutions(ctx):
    rl, ru, _, _ = golomb_roots(ctx, 16)
    both(lambda steal, info: ctx.dfs_forest(rl, ru, small=True, steps_per_launch=16, capacity=64, collect_solutions=True, sink_capacity=8, steal=steal, info=info),
         "golomb6 collect", full_sink=True)
    _, _, infos = both(lambda steal, info: ctx.dfs_forest(rl, ru, small=True, steps_per_launch=16, capacity=64, collect_solutions=True, sink_capacity=1 << 17,
                                                          steal=steal, info=info), "golomb6 collect, roomy sink")
    assert infos["host"]["drains"] == 0 and infos["device"]["drains"] == 0  # (it never filled: that is the case's premise)


def test_golomb_stacks_grow_between_steals(ctx):
    """Two-row stacks: ForestStacks.grow re-points the state in mid-search, and the stealer has to move rows in the grown buffers."""
    rl, ru, _, _ = golomb_roots(ctx, 16)
    h, d, infos = both(lambda steal, info: ctx.dfs_forest(rl, ru, small=True, steps_per_launch=8, capacity=2, max_capacity=256, steal=steal, info=info), "golomb6 grow")
    assert infos["host"]["grown"] > 0 and infos["device"]["grown"] == infos["host"]["grown"]


# ------------------------------------------------------------------------------------------------ the five-task schedule, the formula-store forest
@pytest.mark.parametrize("brancher", ["split", "enumerate"])
def test_schedule_formula_store(ctx, brancher):
    vs, cs, _ = FC.schedule("B5")
    lb0, ub0 = push_store(ctx, vs, cs)
    if brancher == "split":
        rl, ru, _ = roots_of(ctx, lb0, ub0, 12)
        run = lambda steal, info: ctx.dfs_forest(rl, ru, formulas=True, steps_per_launch=8, capacity=64, steal=steal, info=info)
    else:
        rl, ru, lists = roots_of(ctx, lb0, ub0, 12, val="middle")
        run = lambda steal, info: ctx.dfs_forest_enum(rl, ru, val="middle", root_excl=lists, forest="form", steps_per_launch=8, capacity=64, steal=steal, info=info)
    both(run, ("B5", brancher))


# ------------------------------------------------------------------------------------------------ the drivers above the context
def test_search_forest_drivers_pass_it_through(ctx):
    from pcp_amd.search_forest import forest_bnb, forest_enumerate, forest_search, forest_solutions
    vs, cs, var = SC.golomb(6)
    lb0, ub0 = push_store(ctx, vs, cs)
    for steal in ("host", "device"):
        ih, kw = {}, dict(n_trees=16, steps_per_launch=16, capacity=64, small=True)
        a = forest_search(ctx, lb0, ub0, steal=steal, info=ih, **kw)
        assert ih["steals"] > 0
        b = forest_enumerate(ctx, lb0, ub0, n_trees=16, steps_per_launch=16, capacity=64, steal=steal)
        c = forest_bnb(ctx, lb0, ub0, (var, "min"), steal=steal, **kw)
        s = forest_solutions(ctx, lb0, ub0, n_trees=16, steps_per_launch=16, capacity=64, steal=steal)
        assert a["error"] == b["error"] == c["error"] == s["error"] == 0
        assert a["solutions"] == b["solutions"] == s["solutions"] == len(s["solutions_lb"]) and c["best"] == SC.OPTIMUM[6]
        if steal == "host":
            first = (a["nodes"], a["solutions"], a["failed"]), (b["nodes"], b["solutions"], b["failed"])
        else:
            assert first == ((a["nodes"], a["solutions"], a["failed"]), (b["nodes"], b["solutions"], b["failed"]))


# ------------------------------------------------------------------------------------------------ refusals
class TwoRanks:
    @staticmethod
    def get_world_size():
        return 2

    @staticmethod
    def get_rank():
        return 0


def test_refusals(ctx):
    from pcp_amd.search_forest import forest_bnb, forest_enumerate, forest_search, forest_solutions
    lb0, ub0 = push_queens(ctx)
    rl, ru = lb0[None], ub0[None]
    with pytest.raises(ValueError, match="one rank"):
        ctx.dfs_forest(rl, ru, steal="device", dist=TwoRanks)
    with pytest.raises(ValueError, match="one rank"):
        ctx.dfs_forest_bnb(rl, ru, (0, "min"), small=True, steal="device", dist=TwoRanks)
    for call in (lambda: ctx.dfs_forest(rl, ru, steal="bogus"),
                 lambda: ctx.dfs_forest_bnb(rl, ru, (0, "min"), small=True, steal="bogus"),
                 lambda: ctx.dfs_forest_enum(rl, ru, steal="bogus"),
                 lambda: ctx.dfs_forest_neq_solutions(rl, ru, steal="bogus"),
                 lambda: forest_search(ctx, lb0, ub0, steal="bogus"),
                 lambda: forest_bnb(ctx, lb0, ub0, (0, "min"), small=True, steal="bogus"),
                 lambda: forest_enumerate(ctx, lb0, ub0, steal="bogus"),
                 lambda: forest_solutions(ctx, lb0, ub0, steal="bogus")):
        with pytest.raises(ValueError, match="steal must be"):
            call()
