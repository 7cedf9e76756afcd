"""Option "var_select" = PCP_VAR_INPUT_ORDER in the search loops on the device, against the host specification (pcp_amd.search with
var_select="input_order" over oracle-backed stand-ins, which test_var_select_cpu.py checks against a restatement and brute force): the
stepping loop pcp_dfs_device, the row-stack forests of Interval stores (formula units, small stores; BinarySplit, Enumerate, branch and
bound, the solution sink), the set-mode forests (plain and formula stores, branch and bound, split refills) and DeviceSearch.  One tree is
the host specification node for node; several trees find the same solutions and the same optimum.  Integer work: no tolerance anywhere."""
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
import setform_forest_ref as R
import small_excl_cases as SX
import var_select_cases as VC
from oracle_ctx import OracleCtx
from test_enum_search_cpu import EnumOracleCtx
from test_form_excl_cpu import FormExclOracleCtx
from test_small_excl_cpu import SmallExclOracleCtx

pytestmark = pytest.mark.gpu

IO = "input_order"
N = 6  # N-queens 6: 4 solutions


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


def counts(r):
    if isinstance(r, dict):
        assert r["error"] == 0, r
        return r["nodes"], r["solutions"], r["failed"]
    return r.num_nodes, r.num_solution, r.num_failed_node


def rows(*a):
    return tuple(np.ascontiguousarray(x, np.int32)[None] for x in a)


def queens():
    return M.nqueens_props(N), np.ones(N, np.int32), np.full(N, N, np.int32)


# ------------------------------------------------------------------------------------------------ the stepping loop
def _stepping_is_the_host(ctx, V, props, lb0, ub0):
    """pcp_dfs_device under InputOrder: the counters and the first solution of search.dfs(var_select="input_order"); a FirstSmallestVar run
    differs; with a stack one row short of sufficient error 1, and the open rows searched as roots of their own give the totals."""
    host = S.dfs(OracleCtx(V, props), lb0, ub0, all_solutions=True, var_select=IO)
    other = S.dfs(OracleCtx(V, props), lb0, ub0, all_solutions=True)
    assert counts(host) != counts(other) and host.num_solution == other.num_solution
    ctx.var_select = IO
    try:
        r = ctx.dfs_device(lb0, ub0, 4000, capacity=64, stop_on_solution=False, chunk=97)
        assert counts(r) == counts(host) and r["open"] == 0, (r, counts(host))
        first = ctx.dfs_device(lb0, ub0, 4000, capacity=64, stop_on_solution=True, chunk=97)
        assert first["solutions"] == 1 and np.array_equal(first["first_solution"], host.solutions[0])
        cap = next(c for c in range(2, 64) if ctx.dfs_device(lb0, ub0, 4000, capacity=c, stop_on_solution=False, chunk=97)["error"] == 0)
        assert cap > 2
        info = {}
        short = ctx.dfs_device(lb0, ub0, 4000, capacity=cap - 1, stop_on_solution=False, chunk=97, info=info)
        assert short["error"] == 1 and short["stopped"] and short["open"] > 0
        total = np.array([short["nodes"], short["solutions"], short["failed"]])
        L, U = info["rows"]
        for row in range(short["open"]):
            sub = ctx.dfs_device(L[row], U[row], 4000, capacity=64, stop_on_solution=False, chunk=97)
            total += counts(sub)
        assert tuple(total.tolist()) == counts(host)
    finally:
        ctx.var_select = "first_smallest"
    r = ctx.dfs_device(lb0, ub0, 4000, capacity=64, stop_on_solution=False, chunk=97)
    assert counts(r) == counts(other)  # the option is not sticky


def test_stepping_loop_on_a_small_model(ctx):
    V, props, lb0, ub0, _ = SX.golomb(5, 11)
    ctx.set_model(V, props)
    _stepping_is_the_host(ctx, V, props, lb0, ub0)


def test_stepping_loop_on_an_all_xneqy_model(ctx):
    props, lb0, ub0 = queens()
    ctx.set_model(N, props)
    _stepping_is_the_host(ctx, N, props, lb0, ub0)


# ------------------------------------------------------------------------------------------------ row-stack forests: formula stores
def test_formula_forest_enumerate_on_the_two_robot_model(ctx):
    """pcp_dfs_forest_device_form_enum, one tree, one solution, MinVal: the search the reference's scheduling example writes down."""
    vs, cs, starts, _, lb0, ub0, pushes, sums = VC.robot(2, 500)
    VC.push_store(ctx, len(vs), pushes, sums)
    r = ctx.dfs_forest_enum(*rows(lb0, ub0), val="min", stop_on_solution=True, want_solution=True, steps_per_launch=16, var_select=IO)
    assert ctx.last_plan()["path"] == 3 and ctx.var_select == "first_smallest"
    print("robot 2/500 on the device:", counts(r), r["first_solutions"][0][starts[:5]].tolist())
    assert (r["nodes"], r["failed"], r["solutions"]) == (VC.ROBOT_PINNED["nodes"], VC.ROBOT_PINNED["failed"], 1)
    assert r["first_solutions"][0][starts[:5]].tolist() == VC.ROBOT_PINNED["starts"]
    fs = ctx.dfs_forest_enum(*rows(lb0, ub0), val="min", stop_on_solution=True, want_solution=True, steps_per_launch=16)
    assert counts(fs) != counts(r)  # FirstSmallestVar's tree is another one


def test_formula_forest_on_A4_all_solutions(ctx):
    vs, cs, _ = FC.schedule("A4")
    lb0, ub0 = vs.bounds()
    M.push_model(ctx, cs, len(vs))
    split = S.dfs(FC.FormulaOracleCtx(vs, cs), lb0, ub0, all_solutions=True, var_select=IO)
    r = ctx.dfs_forest(*rows(lb0, ub0), formulas=True, steps_per_launch=32, var_select=IO)
    assert counts(r) == counts(split) != counts(S.dfs(FC.FormulaOracleCtx(vs, cs), lb0, ub0, all_solutions=True))
    for val in ("middle", "min"):
        host = S.dfs_enumerate(VC.StoreOracleCtx(vs, cs), lb0, ub0, all_solutions=True, val=val, var_select=IO)
        r = ctx.dfs_forest_enum(*rows(lb0, ub0), val=val, steps_per_launch=32, var_select=IO)
        assert counts(r) == counts(host), val
        for n_trees in (2, 8):  # expansion plus trees: the same solutions
            f = SF.forest_enumerate(ctx, lb0, ub0, val=val, n_trees=n_trees, steps_per_launch=8, var_select=IO)
            assert f["error"] == 0 and f["solutions"] == host.num_solution, (val, n_trees)
    for n_trees in (2, 8):
        f = SF.forest_search(ctx, lb0, ub0, n_trees=n_trees, steps_per_launch=8, formulas=True, var_select=IO)
        assert f["error"] == 0 and f["solutions"] == split.num_solution, n_trees


def test_formula_forest_sink_under_input_order(ctx):
    """collect_solutions with a sink one row short of the solution count: drained on the way, the boxes are brute force's schedules."""
    vs, cs, _ = FC.schedule("A4")
    lb0, ub0 = vs.bounds()
    M.push_model(ctx, cs, len(vs))
    truth = X.all_schedules("A4")
    n = ctx.dfs_forest_enum(*rows(lb0, ub0), val="min", steps_per_launch=32, var_select=IO)["solutions"]
    info = {}
    r = ctx.dfs_forest_enum(*rows(lb0, ub0), val="min", steps_per_launch=32, collect_solutions=True, sink_capacity=n - 1, info=info, var_select=IO)
    got, total = X.covered(4, list(zip(r["solutions_lb"], r["solutions_ub"])))
    assert r["solutions"] == n == len(r["solutions_lb"]) and info["drains"] >= 1 and got == set(truth) and total == len(truth)


def test_formula_forest_branch_and_bound_on_C4mk(ctx):
    key = "search:C4mk"
    vs, cs, mk, lb0, ub0, _, _ = X.store(key)
    X.push(ctx, key)
    host = S.dfs(FC.FormulaOracleCtx(vs, cs), lb0, ub0, objective=(mk, "min"), var_select=IO)
    r = ctx.dfs_forest_bnb(*rows(lb0, ub0), (mk, "min"), steps_per_launch=32, var_select=IO)
    assert counts(r) == counts(host) and r["best"] == host.best and np.array_equal(r["best_solution"], host.best_solution)
    for val in ("middle", "min"):
        host = S.dfs_enumerate(FormExclOracleCtx(key), lb0, ub0, val=val, objective=(mk, "min"), var_select=IO)
        r = ctx.dfs_forest_enum(*rows(lb0, ub0), val=val, objective=(mk, "min"), steps_per_launch=32, var_select=IO)
        assert counts(r) == counts(host) and r["best"] == host.best and np.array_equal(r["best_solution"], host.best_solution), val
        for n_trees in (2, 8):
            f = SF.forest_enumerate(ctx, lb0, ub0, val=val, objective=(mk, "min"), n_trees=n_trees, steps_per_launch=8, var_select=IO)
            assert f["error"] == 0 and f["best"] == host.best, (val, n_trees)
    for n_trees in (2, 8):
        f = SF.forest_bnb(ctx, lb0, ub0, (mk, "min"), n_trees=n_trees, steps_per_launch=8, var_select=IO)
        assert f["error"] == 0 and f["best"] == host.best


# ------------------------------------------------------------------------------------------------ row-stack forests: small stores
def _small_forest_is_the_host(ctx, V, props, lb0, ub0, var, enum_ctx):
    host = S.dfs(OracleCtx(V, props), lb0, ub0, all_solutions=True, var_select=IO)
    r = ctx.dfs_forest(*rows(lb0, ub0), small=True, steps_per_launch=32, var_select=IO)
    assert ctx.last_plan()["path"] == 4
    assert counts(r) == counts(host) != counts(S.dfs(OracleCtx(V, props), lb0, ub0, all_solutions=True))
    for n_trees in (2, 8):
        f = SF.forest_search(ctx, lb0, ub0, n_trees=n_trees, steps_per_launch=8, small=True, var_select=IO)
        assert f["error"] == 0 and f["solutions"] == host.num_solution
    for val in ("middle", "min"):
        host = S.dfs_enumerate(enum_ctx(), lb0, ub0, all_solutions=True, val=val, var_select=IO)
        r = ctx.dfs_forest(*rows(lb0, ub0), small=True, brancher="enumerate", val=val, steps_per_launch=32, var_select=IO)
        assert counts(r) == counts(host), val
        for n_trees in (2, 8):
            f = SF.forest_search(ctx, lb0, ub0, n_trees=n_trees, steps_per_launch=8, small=True, brancher="enumerate", val=val, var_select=IO)
            assert f["error"] == 0 and f["solutions"] == host.num_solution, (val, n_trees)
    if var is None:
        return
    host = S.dfs(OracleCtx(V, props), lb0, ub0, objective=(var, "min"), var_select=IO)
    r = ctx.dfs_forest_bnb(*rows(lb0, ub0), (var, "min"), small=True, steps_per_launch=32, var_select=IO)
    assert counts(r) == counts(host) and r["best"] == host.best and np.array_equal(r["best_solution"], host.best_solution)
    for val in ("middle", "min"):
        host = S.dfs_enumerate(SmallExclOracleCtx(V, props), lb0, ub0, val=val, objective=(var, "min"), var_select=IO)
        r = ctx.dfs_forest_bnb(*rows(lb0, ub0), (var, "min"), small=True, brancher="enumerate", val=val, steps_per_launch=32, var_select=IO)
        assert counts(r) == counts(host) and r["best"] == host.best and np.array_equal(r["best_solution"], host.best_solution), val
    for n_trees in (2, 8):
        f = SF.forest_bnb(ctx, lb0, ub0, (var, "min"), n_trees=n_trees, steps_per_launch=8, small=True, var_select=IO)
        assert f["error"] == 0 and f["best"] == host.best


def test_small_forest_on_golomb_5(ctx):
    V, props, lb0, ub0, var = SX.golomb(5, 11)
    ctx.set_model(V, props)
    _small_forest_is_the_host(ctx, V, props, lb0, ub0, var, lambda: SmallExclOracleCtx(V, props))


def test_small_forest_on_nqueens_6(ctx):
    props, lb0, ub0 = queens()
    ctx.set_model(N, props)
    _small_forest_is_the_host(ctx, N, props, lb0, ub0, None, lambda: EnumOracleCtx(N, props))
    with pytest.raises(ValueError, match="all-XNeqY"):  # the in-kernel all-XNeqY forest selects FirstSmallestVar only
        SF.forest_search(ctx, lb0, ub0, n_trees=2, var_select=IO)
    assert ctx.var_select == "first_smallest"


# ------------------------------------------------------------------------------------------------ set forests
BRANCHERS = (("split", "middle"), ("enumerate", "middle"), ("enumerate", "min"))


def _host_set(sctx, lb0, ub0, base, brancher, val, **kw):
    if brancher == "split":
        return S.dfs_set(sctx, lb0, ub0, base, var_select=IO, **kw)
    return S.dfs_enumerate_set(sctx, lb0, ub0, base, val=val, var_select=IO, **kw)


def test_set_forest_on_nqueens_6(ctx):
    props, sw, lb0, ub0 = ES.nqueens_model(N)
    ctx.set_model(N, props, set_words=sw)
    ctx.set_hull(1, N)
    root = M.interval_bits(lb0, ub0, sw, 1)[None]
    for brancher, val in BRANCHERS:
        host = _host_set(ES.SetOracleCtx(N, props, sw, 1), lb0, ub0, 1, brancher, val, all_solutions=True)
        r = ctx.dfs_forest_set(root, brancher=brancher, val=val, steps_per_launch=16, var_select=IO)
        assert counts(r) == counts(host) and np.array_equal(r["first_solution"], host.solutions[0]), (brancher, val)
        f = SF.forest_search_set(ctx, lb0, ub0, 1, n_trees=4, steps_per_launch=4, brancher=brancher, val=val, var_select=IO)
        assert f["error"] == 0 and f["solutions"] == host.num_solution == 4, (brancher, val)


def test_set_forest_branch_and_bound_on_golomb_5(ctx):
    V, props, lb0, ub0, var = SX.golomb(5, 11)
    ctx.set_model(V, props, set_words=1)
    ctx.set_hull(0, 11)
    root = M.interval_bits(lb0, ub0, 1, 0)[None]
    for brancher, val in BRANCHERS:
        host = _host_set(ES.SetOracleCtx(V, props, 1, 0), lb0, ub0, 0, brancher, val, objective=(var, "min"))
        r = ctx.dfs_forest_set_bnb(root, (var, "min"), brancher=brancher, val=val, steps_per_launch=16, var_select=IO)
        assert counts(r) == counts(host) and r["best"] == host.best == 11 and np.array_equal(r["best_solution"], host.best_solution), (brancher, val)
        f = SF.forest_bnb_set(ctx, lb0, ub0, 0, (var, "min"), n_trees=4, ramp_steps=2, steps_per_launch=8, brancher=brancher, val=val, var_select=IO)
        assert f["error"] == 0 and f["best"] == 11, (brancher, val)


class _SetStoreCtx:
    def __init__(self, vs, cs, base=0):
        self._m, self.n_vars, self.set_words, self.base = SC.oracle_model(vs, cs), len(vs), 1, base
        self.n_units = self._m.n_units

    def propagate_set(self, bits, active=None, want_stats=True):
        lb, ub, b, act, st, s = self._m.consistency_set(bits, self.base, active)
        return lb, ub, b, act, st, {"steps": s["steps"], "steps3": 0}


def test_set_formula_forest_on_the_four_task_schedule(ctx):
    """test_setform_forest_gpu.py's model (four tasks on one machine, horizon 8), with and without the makespan variable."""
    vs, cs, _ = R.schedule(R.DUR4, 8, False)
    lb0, ub0 = vs.bounds()
    M.push_model(ctx, cs, len(vs), 1)
    ctx.set_hull(0, 63)
    root = SC.hull_sets(vs, 1, 0)[None]
    for brancher, val in BRANCHERS:
        host = _host_set(_SetStoreCtx(vs, cs), lb0, ub0, 0, brancher, val, all_solutions=True)
        r = ctx.dfs_forest_setform(root, brancher=brancher, val=val, steps_per_launch=16, var_select=IO)
        assert counts(r) == counts(host), (brancher, val)
        f = SF.forest_search_set(ctx, lb0, ub0, 0, n_trees=4, steps_per_launch=4, brancher=brancher, val=val, formulas=True, var_select=IO)
        assert f["error"] == 0 and f["solutions"] == host.num_solution, (brancher, val)
    vs, cs, m = R.schedule(R.DUR4, 8, True)
    lb0, ub0 = vs.bounds()
    M.push_model(ctx, cs, len(vs), 1)
    ctx.set_hull(0, 63)
    root = SC.hull_sets(vs, 1, 0)[None]
    for brancher, val in BRANCHERS:
        host = _host_set(_SetStoreCtx(vs, cs), lb0, ub0, 0, brancher, val, objective=(m, "min"))
        r = ctx.dfs_forest_setform_bnb(root, (m, "min"), brancher=brancher, val=val, steps_per_launch=16, var_select=IO)
        assert counts(r) == counts(host) and r["best"] == host.best and np.array_equal(r["best_solution"], host.best_solution), (brancher, val)
        f = SF.forest_bnb_set(ctx, lb0, ub0, 0, (m, "min"), n_trees=4, ramp_steps=2, steps_per_launch=8, brancher=brancher, val=val, formulas=True, var_select=IO)
        assert f["error"] == 0 and f["best"] == host.best, (brancher, val)


# ------------------------------------------------------------------------------------------------ DeviceSearch
def test_device_search_on_the_two_robot_model_and_on_A4(ctx):
    vs, cs, starts, _, lb0, ub0, pushes, sums = VC.robot(2, 500)
    VC.push_store(ctx, len(vs), pushes, sums)
    st = DeviceSearch(ctx, batch=1, implicit=True, brancher="enumerate", val="min", var_select=IO).run(lb0, ub0, all_solutions=False, keep_solutions=1)
    assert (st.num_nodes, st.num_failed_node, st.num_solution) == (VC.ROBOT_PINNED["nodes"], VC.ROBOT_PINNED["failed"], 1)
    assert st.solutions[0][starts[:5]].tolist() == VC.ROBOT_PINNED["starts"] and ctx.var_select == "first_smallest"
    vs, cs, _ = FC.schedule("A4")
    lb0, ub0 = vs.bounds()
    M.push_model(ctx, cs, len(vs))
    truth = X.all_schedules("A4")
    for batch in (4, 256):
        host = S.dfs_enumerate(VC.StoreOracleCtx(vs, cs), lb0, ub0, all_solutions=True, batch=batch, val="min", var_select=IO)
        ds = DeviceSearch(ctx, batch=batch, implicit=True, brancher="enumerate", val="min", var_select=IO)
        ds.reset(lb0, ub0)
        ds.advance(all_solutions=True, keep_solutions=1 << 20, keep_bounds=True)
        got, total = X.covered(4, list(zip(ds.stats.solutions, ds.solutions_ub)))
        assert counts(ds.stats) == counts(host) and got == set(truth) and total == len(truth), batch


def test_device_search_in_set_mode(ctx):
    props, sw, lb0, ub0 = ES.nqueens_model(N)
    ctx.set_model(N, props, set_words=sw)
    ctx.set_hull(1, N)
    truth = VC.brute_queens(N)
    for brancher, val in BRANCHERS:
        for batch in (1, 4, 256):
            host = _host_set(ES.SetOracleCtx(N, props, sw, 1), lb0, ub0, 1, brancher, val, all_solutions=True, batch=batch)
            st = DeviceSearch(ctx, batch=batch, implicit=True, brancher=brancher, val=val, var_select=IO).run(lb0, ub0, keep_solutions=64, base=1)
            assert counts(st) == counts(host) and sorted(tuple(int(x) for x in s) for s in st.solutions) == truth, (brancher, val, batch)
