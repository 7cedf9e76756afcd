"""The variable selector InputOrder (search/branching/input_order.rs:30-39) in the host layers, without a GPU: the selector on the reference's
own vectors, the host specification (pcp_amd.search with var_select="input_order") against a plain restatement on the 2-robot scheduling model
and against brute force on N-queens 6, the schedule A4 and Golomb 5 (Interval stores) and on N-queens 6 and a one-unit disjunction (sets),
at batch sizes 1, 3 and 16; the drivers' ``var_select=`` over stand-in contexts: None touches nothing, a value is set and restored, also
when the run raises; the two refusals."""
import itertools
import os

import numpy as np
import pytest

from pcp_amd import model as M
from pcp_amd import search as S
from pcp_amd import search_forest as SF
from pcp_amd.search_device import DeviceSearch

import enum_set_ref as ES
import form_excl_cases as X
import form_forest_cases as FC
import setform_cases as SC
import small_excl_cases as SX
import var_select_cases as VC
from oracle_ctx import OracleCtx
from test_enum_search_cpu import EnumOracleCtx
from test_small_excl_cpu import SmallExclOracleCtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 3, 16)


# ------------------------------------------------------------------------------------------------ the selector
VECTORS = [  # input_order.rs:48-62
    ([(1, 10), (2, 4), (1, 1)], 0),
    ([(1, 10), (2, 4), (2, 4)], 0),
    ([(1, 1), (1, 1), (1, 10), (1, 1), (2, 4), (1, 1), (1, 1)], 2),
]


@pytest.mark.parametrize("doms,want", VECTORS)
def test_the_reference_vectors(doms, want):
    lb, ub = np.array([[a for a, _ in doms]], np.int32), np.array([[b for _, b in doms]], np.int32)
    assert S.input_order(lb, ub).tolist() == [want] and S.select_var(lb, ub, "input_order").tolist() == [want]
    bits = M.interval_bits(lb, ub, 1, 0)
    assert S.input_order_set(bits).tolist() == [want] and S.select_var_set(bits, "input_order").tolist() == [want]
    assert VC.ref_input_order([b - a + 1 for a, b in doms]) == want


def test_all_assigned_raises_and_unknown_names_are_refused():
    lb = np.array([[1, 1, 1]], np.int32)
    assert S.input_order(lb, lb).tolist() == [-1] and S.input_order_set(M.interval_bits(lb, lb, 1, 0)).tolist() == [-1]
    with pytest.raises(RuntimeError):
        S.branch(lb, lb, None, var_select="input_order")
    with pytest.raises(RuntimeError):
        S.branch_set(M.interval_bits(lb, lb, 1, 0), lb, lb, 0, None, var_select="input_order")
    for call in (lambda: S.branch(lb, lb + 1, None, var_select="smallest"), lambda: S.branch_set(M.interval_bits(lb, lb + 1, 1, 0), lb, lb + 1, 0, None, var_select="x"),
                 lambda: S.dfs(None, lb[0], lb[0], var_select="first"), lambda: S.dfs_set(None, lb[0], lb[0], 0, var_select="first"),
                 lambda: S.dfs_enumerate_set(None, lb[0], lb[0], 0, var_select="first")):
        with pytest.raises(ValueError):
            call()
    # the set form counts members, not the width of the bounds: {0, 9} has two values, {5} one
    bits = np.zeros((1, 2, 1), np.uint64)
    bits[0, 0, 0], bits[0, 1, 0] = 1 << 5, (1 << 0) | (1 << 9)
    assert S.input_order_set(bits).tolist() == [1]


def test_the_constants_in_the_header_the_engine_and_the_rust_binding():
    import pcp_amd.engine as E
    header = open(os.path.join(ROOT, "include", "pcp_hip.h")).read()
    rust = open(os.path.join(ROOT, "integration", "pcp-hip-sys", "src", "lib.rs")).read()
    assert "#define PCP_VAR_FIRST_SMALLEST 0u" in header and "#define PCP_VAR_INPUT_ORDER 1u" in header and "#define PCP_ABI_VERSION 8" in header
    assert "PCP_VAR_FIRST_SMALLEST: u32 = 0" in rust and "PCP_VAR_INPUT_ORDER: u32 = 1" in rust
    assert E.VAR_SELECTS == {"first_smallest": 0, "input_order": 1}


# ------------------------------------------------------------------------------------------------ the robot model against a restatement
def test_robot_scheduling_is_the_reference_model():
    vs, cs, starts, durations, lb0, ub0, _, _ = VC.robot(2, 500)
    assert len(vs) == 42 and starts == [0, 1, 2, 3, 4, 9, 10, 11, 12, 13] and durations == [5, 6, 7, 8, 14, 15, 16, 17]
    assert lb0[starts].tolist() == [1] * 10 and ub0[starts].tolist() == [500] * 10
    assert list(zip(lb0[durations[:4]].tolist(), ub0[durations[:4]].tolist())) == [(10, 15), (25, 35), (240, 250), (25, 35)]
    assert len(M.robot_scheduling(3, 1000)[0]) == 87


def test_the_host_specification_on_the_two_robot_model_is_the_restatement():
    """dfs_enumerate(var_select="input_order", val="min"), one solution, against the plain loop of var_select_cases.restate_enumerate: nodes,
    failed nodes, the first solution's lower bounds; pinned.  FirstSmallestVar walks another tree on the same model."""
    vs, cs, starts, _, lb0, ub0, _, _ = VC.robot(2, 500)
    ctx = VC.StoreOracleCtx(vs, cs)
    ref = VC.restate_enumerate(ctx, lb0, ub0, VC.ref_input_order)
    host = S.dfs_enumerate(ctx, lb0, ub0, val="min", var_select="input_order")
    print("robot 2/500 input_order:", ref["nodes"], ref["failed"], ref["first"][starts[:5]].tolist())
    assert (host.num_nodes, host.num_failed_node, host.num_solution) == (ref["nodes"], ref["failed"], 1) and ctx.form_calls > 0
    assert np.array_equal(host.solutions[0], ref["first"])
    assert (ref["nodes"], ref["failed"]) == (VC.ROBOT_PINNED["nodes"], VC.ROBOT_PINNED["failed"])
    assert ref["first"][starts[:5]].tolist() == VC.ROBOT_PINNED["starts"]
    other = VC.restate_enumerate(ctx, lb0, ub0, VC.ref_first_smallest)
    fs = S.dfs_enumerate(ctx, lb0, ub0, val="min")
    print("robot 2/500 first_smallest:", other["nodes"], other["failed"], other["first"][starts[:5]].tolist())
    assert (fs.num_nodes, fs.num_failed_node) == (other["nodes"], other["failed"]) and np.array_equal(fs.solutions[0], other["first"])
    assert other["nodes"] != ref["nodes"] and not np.array_equal(other["first"], ref["first"])
    # the first solution is a schedule: precedences hold and the Loading / Put tasks of the two robots never overlap
    row = ref["first"]
    tasks = [(int(row[s]), int(row[s]) + int(row[d])) for s, d in ((0, 5), (3, 8), (9, 14), (12, 17))]
    assert all(a1 <= b0 or a0 >= b1 for (a0, a1), (b0, b1) in itertools.combinations(tasks, 2))


# ------------------------------------------------------------------------------------------------ against brute force, Interval stores
def _recorded(ctx):
    """ctx.propagate, recording the box of every Satisfiable node."""
    boxes, inner = [], ctx.propagate

    def propagate(lb, ub, active=None, want_stats=True):
        r = inner(lb, ub, active, want_stats)
        boxes.extend((r[0][i].copy(), r[1][i].copy()) for i in np.nonzero(r[3] == M.TRUE)[0])
        return r
    ctx.propagate = propagate
    return boxes


@pytest.mark.parametrize("batch", BATCHES)
def test_nqueens_6_under_both_distributors(batch):
    n, truth = 6, VC.brute_queens(6)
    props = M.nqueens_props(n)
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    assert len(truth) == 4
    st = S.dfs(OracleCtx(n, props), lb0, ub0, all_solutions=True, batch=batch, var_select="input_order")
    assert sorted(tuple(int(x) for x in s) for s in st.solutions) == truth
    for val in ("middle", "min"):
        st = S.dfs_enumerate(EnumOracleCtx(n, props), lb0, ub0, all_solutions=True, batch=batch, val=val, var_select="input_order")
        assert sorted(tuple(int(x) for x in s) for s in st.solutions) == truth, val


@pytest.mark.parametrize("batch", BATCHES)
def test_the_schedule_A4_under_both_distributors(batch):
    """Satisfiable nodes of an Interval store are boxes: together they hold every schedule of the model exactly once."""
    vs, cs, _ = FC.schedule("A4")
    lb0, ub0 = vs.bounds()
    truth = X.all_schedules("A4")
    ctx = FC.FormulaOracleCtx(vs, cs)
    boxes = _recorded(ctx)
    st = S.dfs(ctx, lb0, ub0, all_solutions=True, batch=batch, var_select="input_order")
    got, total = X.covered(4, boxes)
    assert st.num_solution == len(boxes) and got == set(truth) and total == len(truth)
    for val in ("middle", "min"):
        rec = []
        st = S.dfs_enumerate(VC.StoreOracleCtx(vs, cs), lb0, ub0, all_solutions=True, batch=batch, val=val, var_select="input_order", record=rec)
        got, total = X.covered(4, [(r[4], r[5]) for r in rec if r[3] == M.TRUE])
        assert got == set(truth) and total == len(truth), val


def _golomb_optimum(m, length):
    best = None
    for marks in itertools.combinations(range(1, length + 1), m - 1):
        mk = (0,) + marks
        d = [mk[j] - mk[i] for i in range(m) for j in range(i + 1, m)]
        if len(set(d)) == len(d) and mk[1] - mk[0] < mk[-1] - mk[-2]:
            best = mk[-1] if best is None else min(best, mk[-1])
    return best


@pytest.mark.parametrize("batch", BATCHES)
def test_golomb_5_minimised_under_both_distributors(batch):
    V, props, lb0, ub0, var = SX.golomb(5, 11)
    want = _golomb_optimum(5, 11)
    assert want == 11
    st = S.dfs(OracleCtx(V, props), lb0, ub0, batch=batch, objective=(var, "min"), var_select="input_order")
    assert st.best == want and int(st.best_solution[var]) == want
    for val in ("middle", "min"):
        st = S.dfs_enumerate(SmallExclOracleCtx(V, props), lb0, ub0, batch=batch, val=val, objective=(var, "min"), var_select="input_order")
        assert st.best == want and int(st.best_solution[var]) == want, val


# ------------------------------------------------------------------------------------------------ set mode
class _SetStoreCtx:
    """propagate_set over the oracle on any lowered store; the sets of every Satisfiable node are recorded."""

    def __init__(self, vs, cs, sw, base):
        self._m, self.n_vars, self.set_words, self.base, self.boxes = SC.oracle_model(vs, cs), len(vs), sw, base, []
        self.n_units = self._m.n_units

    def propagate_set(self, bits, active=None, want_stats=True):
        lb, ub, b, act, st, s = self._m.consistency_set(bits, self.base, active)
        self.boxes += [b[i].copy() for i in np.nonzero(st == M.TRUE)[0]]
        return lb, ub, b, act, st, {"steps": s["steps"], "steps3": 0}


@pytest.mark.parametrize("batch", BATCHES)
def test_set_mode_nqueens_6(batch):
    n, truth = 6, VC.brute_queens(6)
    props, sw, lb0, ub0 = ES.nqueens_model(n)
    st = S.dfs_set(ES.SetOracleCtx(n, props, sw, 1), lb0, ub0, 1, all_solutions=True, batch=batch, var_select="input_order")
    assert sorted(tuple(int(x) for x in s) for s in st.solutions) == truth
    for val in ("middle", "min"):
        st = S.dfs_enumerate_set(ES.SetOracleCtx(n, props, sw, 1), lb0, ub0, 1, all_solutions=True, batch=batch, val=val, var_select="input_order")
        assert sorted(tuple(int(x) for x in s) for s in st.solutions) == truth, val


@pytest.mark.parametrize("batch", BATCHES)
def test_set_mode_one_unit_disjunction(batch):
    """setform_cases.hand_or_eq_bool from its hull: x in 1..5, y in 2..4, b in 0..1 under Or(x = y, Boolean(b)).  The Satisfiable nodes'
    sets hold every solution exactly once."""
    vs, cs, _ = SC.hand_or_eq_bool()
    lb0, ub0 = vs.bounds()
    truth = {(x, y, b) for x in range(1, 6) for y in range(2, 5) for b in (0, 1) if x == y or b == 1}

    def points(boxes):
        return [p for bx in boxes for p in itertools.product(*(S.set_members(bx[v], 0).tolist() for v in range(3)))]
    runs = [lambda c: S.dfs_set(c, lb0, ub0, 0, all_solutions=True, batch=batch, var_select="input_order")]
    runs += [lambda c, val=val: S.dfs_enumerate_set(c, lb0, ub0, 0, all_solutions=True, batch=batch, val=val, var_select="input_order") for val in ("middle", "min")]
    for run in runs:
        ctx = _SetStoreCtx(vs, cs, 1, 0)
        st = run(ctx)
        pts = points(ctx.boxes)
        assert st.num_solution == len(ctx.boxes) and set(pts) == truth and len(pts) == len(truth)


# ------------------------------------------------------------------------------------------------ the drivers over stand-in contexts
def _queens_search(ctx, **kw):
    import torch
    return DeviceSearch(ctx, batch=4, device=torch.device("cpu"), implicit=True, **kw)


def test_device_search_none_touches_nothing_and_a_value_is_set_and_restored():
    n, truth = 6, VC.brute_queens(6)
    props = M.nqueens_props(n)
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    # None: a context without the attribute runs as before, and the option is never set
    plain = VC.VSEnumOracleCtx(n, props)
    st = _queens_search(plain, brancher="enumerate", val="min").run(lb0, ub0, keep_solutions=64)
    assert "var_select" not in plain.option_keys and not hasattr(plain, "var_select_log") and st.num_solution == 4
    old = EnumOracleCtx(n, props)  # (a stand-in from before the option: no var_select at all)
    assert _queens_search(old, brancher="enumerate", val="min").run(lb0, ub0).num_solution == 4
    # a value: set for the run, restored afterwards; the tree is the host specification's at batch 4
    for brancher, host in (("split", lambda: S.dfs(OracleCtx(n, props), lb0, ub0, all_solutions=True, batch=4, var_select="input_order")),
                           ("enumerate", lambda: S.dfs_enumerate(EnumOracleCtx(n, props), lb0, ub0, all_solutions=True, batch=4, val="min", var_select="input_order"))):
        ctx = VC.VSEnumOracleCtx(n, props)
        st = _queens_search(ctx, brancher=brancher, val="min", var_select="input_order").run(lb0, ub0, keep_solutions=64)
        h = host()
        assert ctx.var_select_log == ["input_order", "first_smallest"] and ctx.var_select == "first_smallest"
        assert (st.num_nodes, st.num_solution, st.num_failed_node) == (h.num_nodes, h.num_solution, h.num_failed_node), brancher
        assert sorted(tuple(int(x) for x in s) for s in st.solutions) == truth
    fs = S.dfs_enumerate(EnumOracleCtx(n, props), lb0, ub0, all_solutions=True, batch=4, val="min")
    assert fs.num_nodes != h.num_nodes  # the selector changes the tree
    # ... also when the run raises (a context set to InputOrder before: that is what comes back)
    ctx = VC.VSEnumOracleCtx(n, props)
    ctx.var_select = "input_order"
    ds = _queens_search(ctx, brancher="enumerate", val="min", var_select="first_smallest")
    ctx.branch_device_excl = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom"))
    with pytest.raises(RuntimeError, match="boom"):
        ds.run(lb0, ub0)
    assert ctx.var_select_log == ["input_order", "first_smallest", "input_order"] and ctx.var_select == "input_order"


def test_device_search_in_set_mode_and_on_the_two_robot_model():
    import torch
    n, truth = 6, VC.brute_queens(6)
    props, sw, lb0, ub0 = ES.nqueens_model(n)
    for brancher in ("split", "enumerate"):
        ctx = VC.VSSetOracleDeviceCtx(n, props, sw, 1)
        st = _queens_search(ctx, brancher=brancher, val="min", var_select="input_order").run(lb0, ub0, keep_solutions=64, base=1)
        host = (S.dfs_set if brancher == "split" else lambda *a, **k: S.dfs_enumerate_set(*a, val="min", **k))(
            ES.SetOracleCtx(n, props, sw, 1), lb0, ub0, 1, all_solutions=True, batch=4, var_select="input_order")
        assert (st.num_nodes, st.num_solution, st.num_failed_node) == (host.num_nodes, host.num_solution, host.num_failed_node), brancher
        assert sorted(tuple(int(x) for x in s) for s in st.solutions) == truth and ctx.var_select_log == ["input_order", "first_smallest"]
    vs, cs, starts, _, rl, ru, _, _ = VC.robot(2, 500)
    ctx = VC.StoreOracleCtx(vs, cs)
    ds = DeviceSearch(ctx, batch=1, device=torch.device("cpu"), implicit=True, brancher="enumerate", val="min", var_select="input_order")
    st = ds.run(rl, ru, all_solutions=False, keep_solutions=1)
    assert (st.num_nodes, st.num_failed_node) == (VC.ROBOT_PINNED["nodes"], VC.ROBOT_PINNED["failed"])
    assert st.solutions[0][starts[:5]].tolist() == VC.ROBOT_PINNED["starts"]


def test_the_new_refusals_and_the_old_one():
    import torch
    n = 6
    props = M.nqueens_props(n)
    ctx = VC.VSEnumOracleCtx(n, props)
    with pytest.raises(ValueError, match="cells"):
        DeviceSearch(ctx, batch=4, device=torch.device("cpu"), implicit=True, cells=True, var_select="input_order")
    with pytest.raises(ValueError, match="var_select"):
        DeviceSearch(ctx, batch=4, device=torch.device("cpu"), implicit=True, var_select="input")
    with pytest.raises(ValueError):  # the selector is not a brancher
        DeviceSearch(ctx, batch=4, device=torch.device("cpu"), implicit=True, brancher="input_order")
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    import pcp_amd.engine as E
    for call in (lambda: SF.forest_search(ctx, lb0, ub0, var_select="input_order"),
                 lambda: E.Context.dfs_forest(ctx, lb0[None], ub0[None], var_select="input_order")):
        with pytest.raises(ValueError, match="all-XNeqY"):
            call()
    with pytest.raises(ValueError, match="var_select"):
        SF.forest_search(ctx, lb0, ub0, small=True, var_select="largest")
    assert not hasattr(ctx, "var_select_log")  # refused before the context was touched


class _Boom(Exception):
    pass


class _ForestStandIn(VC.VarSelectStandIn):
    """A context whose every forest entry raises: what the drivers do around the run is all that is looked at."""
    n_vars, set_words, has_formulas, words, device = 6, 1, False, 0, "cpu"

    def __getattr__(self, name):
        if name.startswith("dfs_forest") or name in ("stats_reset", "propagate_device", "set_model"):
            def boom(*a, **k):
                raise _Boom(name)
            return boom
        raise AttributeError(name)

    def set_option(self, key, value):
        self.__dict__.setdefault("option_keys", []).append(key)


def test_the_forest_drivers_set_and_restore_also_when_the_run_raises():
    import pcp_amd.engine as E
    lb0, ub0 = np.ones(6, np.int32), np.full(6, 6, np.int32)
    roots = np.zeros((1, 6, 1), np.uint64)
    drivers = [
        lambda c, **k: SF.forest_search(c, lb0, ub0, small=True, **k),
        lambda c, **k: SF.forest_bnb(c, lb0, ub0, (0, "min"), small=True, **k),
        lambda c, **k: SF.forest_enumerate(c, lb0, ub0, val="min", **k),
        lambda c, **k: SF.forest_search_set(c, lb0, ub0, 1, **k),
        lambda c, **k: SF.forest_bnb_set(c, lb0, ub0, 1, (0, "min"), **k),
        lambda c, **k: E.Context.dfs_forest(c, lb0[None], ub0[None], small=True, **k),
        lambda c, **k: E.Context.dfs_forest_bnb(c, lb0[None], ub0[None], (0, "min"), small=True, **k),
        lambda c, **k: E.Context.dfs_forest_enum(c, lb0[None], ub0[None], val="min", **k),
        lambda c, **k: E.Context.dfs_forest_set(c, roots, **k),
        lambda c, **k: E.Context.dfs_forest_setform(c, roots, **k),
        lambda c, **k: E.Context.dfs_forest_set_bnb(c, roots, (0, "min"), **k),
        lambda c, **k: E.Context.dfs_forest_setform_bnb(c, roots, (0, "min"), **k),
    ]
    for i, run in enumerate(drivers):
        ctx = _ForestStandIn()
        with pytest.raises(Exception):
            run(ctx)  # var_select=None: whatever the run does, the selector is never read or written
        assert not hasattr(ctx, "var_select_log") and "var_select" not in ctx.__dict__.get("option_keys", []), i
        ctx = _ForestStandIn()
        ctx.var_select = "input_order"
        with pytest.raises(Exception):
            run(ctx, var_select="first_smallest")
        assert ctx.var_select_log == ["input_order", "first_smallest", "input_order"] and ctx.var_select == "input_order", i
