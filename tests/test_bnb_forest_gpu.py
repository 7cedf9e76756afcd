"""pcp_dfs_forest_device_set_bnb: branch and bound (search/branch_and_bound.rs:64-84) inside the set-mode forest kernel — the incumbent is
one device word, folded into the objective's set whenever a tree enters a node.  Against the restatements of the reference's loop over the
CPU oracle (tests/test_bnb_host.py::reference_bnb_set, tests/test_bnb_forest_cpu.py::reference_bnb_set_any):
  * one tree is the reference node for node, under BinarySplit and under Enumerate, for launches so short that every kind of node is
    persisted and resumed;
  * an incumbent seeded by the caller; a fold across a word boundary of a two-word set with a negative base;
  * many trees grown from one root through the split kernel find the optimum of tests/golden/bnb_kats.json;
  * the refusals of the C entry point."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from pcp_amd import model as M
from test_bnb_forest_cpu import CASES, MODELS, reference, reference_bnb_set_any
from test_bnb_host import GOLOMB, reference_bnb_set

pytestmark = pytest.mark.gpu

STEPS = (3, 7, 256)


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    return E.Context(0)


def load(ctx, name):
    """The model on the device over one-word sets with base 0, as the restatements run it."""
    V, props, lb0, ub0, var = MODELS[name][0]()
    assert int(np.min(lb0)) >= 0 and int(np.max(ub0)) < 64
    ctx.set_model(V, props, set_words=1)
    ctx.set_hull(0, int(np.max(ub0)))
    return V, props, lb0, ub0, var


def check_row(props, V, row, var, best, sw=1, base=0):
    """The row that set the incumbent is a solution (the oracle finds the assigned row Satisfiable) and carries the incumbent."""
    assert row is not None and int(row[var]) == best
    _, _, _, _, st, _ = orc.OracleModel(V, props).consistency_set(M.interval_bits(row, row, sw, base)[None], base)
    assert int(st[0]) == M.TRUE


def run_one_tree(ctx, lb0, ub0, var, mode, sw=1, base=0, **kw):
    r = ctx.dfs_forest_set_bnb(M.interval_bits(np.asarray(lb0), np.asarray(ub0), sw, base)[None], (var, mode), **kw)
    assert r["error"] == 0 and r["finished_trees"] == 1 and not r["stopped"]
    assert r["total_nodes"] == r["nodes"]
    return r


def same_search(r, ref):
    print("device", (r["nodes"], r["failed"], r["solutions"], r["best"]), "reference", (ref["nodes"], ref["failed"], ref["solutions"], ref["best"]))
    assert (r["nodes"], r["failed"], r["solutions"], r["best"]) == (ref["nodes"], ref["failed"], ref["solutions"], ref["best"])


@pytest.mark.parametrize("name,mode,opt", CASES)
def test_one_tree_is_the_reference_node_for_node(ctx, name, mode, opt):
    V, props, lb0, ub0, var = load(ctx, name)
    ref = reference_bnb_set(orc.OracleModel(V, props), lb0, ub0, var, mode == "min", 1, 0)
    if opt is not None:
        assert ref["best"] == opt
    if name == "golomb6":
        assert (ref["nodes"], ref["failed"], ref["solutions"], ref["incumbents"]) == (141, 68, 3, [20, 18, 17])
    for steps in STEPS:
        r = run_one_tree(ctx, lb0, ub0, var, mode, steps_per_launch=steps)
        same_search(r, ref)
        check_row(props, V, r["best_solution"], var, ref["best"])
        assert r["tree_best"].tolist() == [ref["best"]]
        assert r["launches"] >= -(-ref["nodes"] // steps)


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("name,mode,opt", CASES)
def test_one_tree_under_enumerate_is_the_reference_node_for_node(ctx, name, mode, opt, val):
    V, props, lb0, ub0, var = load(ctx, name)
    ref = reference(name, mode, "enumerate", val)
    if opt is not None:
        assert ref["best"] == opt
    for steps in STEPS:
        r = run_one_tree(ctx, lb0, ub0, var, mode, steps_per_launch=steps, brancher="enumerate", val=val)
        same_search(r, ref)
        check_row(props, V, r["best_solution"], var, ref["best"])


@pytest.mark.parametrize("brancher", ["split", "enumerate"])
def test_a_seeded_incumbent(ctx, brancher):
    V, props, lb0, ub0, var = load(ctx, "golomb6")
    assert GOLOMB[(6, 30)]["optimum"] == 17
    # nothing beats the optimum itself: every node is entered under var < 17
    ref = reference("golomb6", "min", brancher, "middle", 17)
    assert ref["solutions"] == 0 and ref["best"] == 17
    for steps in (3, 256):
        r = run_one_tree(ctx, lb0, ub0, var, "min", steps_per_launch=steps, best0=17, brancher=brancher)
        same_search(r, ref)
        assert r["best_solution"] is None and r["best"] == 17
    ref = reference("golomb6", "min", brancher, "middle", 18)
    assert ref["best"] == 17 and ref["solutions"] >= 1
    for steps in (3, 256):
        r = run_one_tree(ctx, lb0, ub0, var, "min", steps_per_launch=steps, best0=18, brancher=brancher)
        same_search(r, ref)
        check_row(props, V, r["best_solution"], var, 17)
    # maximize on the reference's own test model (optimum 9)
    V, props, lb0, ub0, var = load(ctx, "kat")
    ref = reference("kat", "max", brancher, "middle", 9)
    assert ref["solutions"] == 0
    r = run_one_tree(ctx, lb0, ub0, var, "max", steps_per_launch=3, best0=9, brancher=brancher)
    same_search(r, ref)
    assert r["best_solution"] is None and r["best"] == 9
    ref = reference("kat", "max", brancher, "middle", 8)
    assert ref["best"] == 9
    r = run_one_tree(ctx, lb0, ub0, var, "max", steps_per_launch=3, best0=8, brancher=brancher)
    same_search(r, ref)
    check_row(props, V, r["best_solution"], var, 9)


def x_less_y(lo, hi):
    vs, cs = M.VStore(), M.CStore()
    x, y = vs.alloc((lo, hi)), vs.alloc((lo, hi))
    cs.alloc(M.XLessY(x, y))
    lb0, ub0 = vs.bounds()
    return cs.lower(2), lb0, ub0


@pytest.mark.parametrize("mode", ["min", "max"])
def test_the_fold_crosses_a_word_boundary(ctx, mode):
    """Two words per set, base -3 (value 61 is bit 0 of the second word): x < y, the objective is x.  Maximizing walks the bound up through
    the word boundary, one value per solution under BinarySplit.
    Under Enumerate the variables are on [-3, 66]: min -> -3, max -> 65.  Under BinarySplit they are on [0, 66] (min -> 0, max -> 65) over
    the same base: on [-3, 66] the reference's own loop does not end — MiddleVal truncates toward zero (middle_val.rs:25-27), so x in
    {-3, -2} gives v = -2 and the left child x <= -2 is the node itself — and neither does the restatement."""
    sw, base, hi = 2, -3, 66
    ctx_hull = (base, hi)
    props, lb0, ub0 = x_less_y(0, hi)
    ref = reference_bnb_set(orc.OracleModel(2, props), lb0, ub0, 0, mode == "min", sw, base)
    assert ref["best"] == (0 if mode == "min" else 65)
    ctx.set_model(2, props, set_words=sw)
    ctx.set_hull(*ctx_hull)
    for steps in (5, 256):
        r = run_one_tree(ctx, lb0, ub0, 0, mode, sw=sw, base=base, steps_per_launch=steps)
        same_search(r, ref)
        check_row(props, 2, r["best_solution"], 0, ref["best"], sw, base)
    props, lb0, ub0 = x_less_y(base, hi)
    ref_e = reference_bnb_set_any(orc.OracleModel(2, props), lb0, ub0, 0, mode == "min", sw, base, "enumerate", "middle")
    assert ref_e["best"] == (-3 if mode == "min" else 65)
    ctx.set_model(2, props, set_words=sw)
    ctx.set_hull(*ctx_hull)
    for steps in (5, 256):
        r = run_one_tree(ctx, lb0, ub0, 0, mode, sw=sw, base=base, steps_per_launch=steps, brancher="enumerate")
        same_search(r, ref_e)
        check_row(props, 2, r["best_solution"], 0, ref_e["best"], sw, base)


@pytest.mark.parametrize("brancher", ["split", "enumerate"])
@pytest.mark.parametrize("n_trees", [8, 64])
def test_many_trees_grown_from_one_root(ctx, n_trees, brancher):
    from pcp_amd.search_forest import forest_bnb_set
    V, props, lb0, ub0, var = load(ctx, "golomb6")
    r = forest_bnb_set(ctx, lb0, ub0, 0, (var, "min"), n_trees=n_trees, ramp_steps=4, steps_per_launch=32, brancher=brancher)
    print(n_trees, brancher, {k: r[k] for k in ("nodes", "failed", "solutions", "splits", "launches", "best")})
    assert r["error"] == 0 and not r["stopped"]
    assert r["best"] == GOLOMB[(6, 30)]["optimum"] == 17
    check_row(props, V, r["best_solution"], var, 17)
    assert int(r["tree_best"].min()) == 17
    assert r["finished_trees"] == n_trees
    assert r["splits"] >= 1
    assert int(r["per_tree"][:, 0].sum()) == r["total_nodes"] == r["nodes"]


def test_refusals(ctx):
    import torch
    import pcp_amd.engine as E
    dev = torch.device("cuda", 0)
    V, props, lb0, ub0, var = load(ctx, "golomb5")
    L, h = ctx._L, ctx._h
    bits = torch.from_numpy(M.interval_bits(np.asarray(lb0), np.asarray(ub0), 1, 0)[None].view(np.int64)).to(dev)
    tree = torch.tensor([[0, 0, -1, 0]], dtype=torch.int32, device=dev)
    levels = torch.zeros((1, 64, 4), dtype=torch.int32, device=dev)
    trail = torch.zeros((1, 1024, 4), dtype=torch.int32, device=dev)
    counters = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    glob = torch.zeros(4, dtype=torch.int64, device=dev)
    best = torch.full((1,), E.no_incumbent("min"), dtype=torch.int32, device=dev)
    tbest = torch.full((1,), E.no_incumbent("min"), dtype=torch.int32, device=dev)
    st = E.ForestState(1, 64, 1024, 0, bits.data_ptr(), tree.data_ptr(), levels.data_ptr(), trail.data_ptr(), counters.data_ptr(), glob.data_ptr(),
                       glob.data_ptr() + 8, None, None)

    def call(var_=var, mode=E.MINIMIZE, best_=best.data_ptr(), tbest_=tbest.data_ptr(), enumerate_=0, val=E.VAL_MIDDLE):
        obj = E.ForestObjective(var_, mode, best_, tbest_, None)
        return L.pcp_dfs_forest_device_set_bnb(h, C.byref(st), C.byref(obj), enumerate_, val, 4, 0, None)

    ERR_ARG = -1
    assert call(var_=V) == ERR_ARG
    assert call(mode=2) == ERR_ARG
    assert call(enumerate_=2) == ERR_ARG
    assert call(val=E.VAL_MIN + 1) == ERR_ARG
    assert call(enumerate_=1, val=E.VAL_MIN + 1) == ERR_ARG
    assert call(best_=None) == ERR_ARG
    assert call(tbest_=None) == ERR_ARG
    assert L.pcp_dfs_forest_device_set_bnb(h, C.byref(st), None, 0, 0, 4, 0, None) == ERR_ARG
    # an interval-mode model: the code of pcp_dfs_forest_device_set
    ctx.set_model(V, props)
    ctx.set_hull(0, int(np.max(ub0)))
    plain = L.pcp_dfs_forest_device_set(h, C.byref(st), 4, 0, 0, None)
    assert plain < 0 and call() == plain
    torch.cuda.synchronize()
    # nothing ran: the state is as it was, and a valid call on the set-mode model then works (tree_row NULL is allowed)
    assert int(counters.sum().item()) == 0 and int(glob[0].item()) == 0
    load(ctx, "golomb5")
    assert call() == 0
    torch.cuda.synchronize()
    assert int(counters[0, 0].item()) == 4 and int(counters[0, 3].item()) == 0
