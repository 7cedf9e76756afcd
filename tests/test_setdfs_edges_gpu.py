"""Two exits of the set-mode search loop on the GPU (-m gpu), on both forests — setdfs_kernel (records, one workgroup per tree) and
setformdfs_kernel (formula units, one wavefront per tree) — under both distributors, one tree each:
  * the level stack is full (error 1): the node that cannot be branched is refused and un-counted, in the tree's counter and in the
    forest's, and what the tree reserved and did not run goes back: total_nodes == nodes;
  * the trail is full (error 4): raised before the node is counted, so the forest's counter keeps the one node that was reserved for it:
    total_nodes - nodes == 1."""
import numpy as np
import pytest

from pcp_amd import model as M

import setform_cases as SC
import setform_forest_ref as R

pytestmark = pytest.mark.gpu

BRANCHERS = ["split", "enumerate"]


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


def records_forest(ctx, brancher, **kw):
    """n-queens 8 over sets, as test_set_forest.test_a_full_trail_is_reported builds it."""
    n = 8
    ctx.set_model(n, M.nqueens_props(n), set_words=1)
    ctx.set_hull(1, n)
    root = M.interval_bits(np.ones(n, np.int32), np.full(n, n, np.int32), 1, 1)[None]
    return ctx.dfs_forest_set(root, steps_per_launch=64, brancher=brancher, val="middle", **kw)


def formula_forest(ctx, brancher, **kw):
    """The four-task schedule of setform_forest_ref (DUR4, horizon 8)."""
    vs, cs, _ = R.schedule(R.DUR4, 8, False)
    M.push_model(ctx, cs, len(vs), 1)
    ctx.set_hull(0, 63)
    return ctx.dfs_forest_setform(SC.hull_sets(vs, 1, 0)[None], brancher=brancher, val="middle", **kw)


@pytest.mark.parametrize("brancher", BRANCHERS)
@pytest.mark.parametrize("forest", [records_forest, formula_forest])
def test_a_full_level_stack_is_reported(ctx, forest, brancher):
    r = forest(ctx, brancher, level_capacity=2)
    print("level stack", forest.__name__, brancher, r["error"], r["stopped"], r["nodes"], r["total_nodes"])
    assert r["error"] == 1 and r["stopped"]
    assert r["nodes"] > 0 and r["total_nodes"] == r["nodes"] == int(r["per_tree"][0, 0])


@pytest.mark.parametrize("brancher", BRANCHERS)
@pytest.mark.parametrize("forest,trail_capacity", [(records_forest, 8), (formula_forest, 4)])
def test_a_full_trail_is_reported(ctx, forest, trail_capacity, brancher):
    r = forest(ctx, brancher, trail_capacity=trail_capacity)
    print("trail", forest.__name__, brancher, r["error"], r["stopped"], r["nodes"], r["total_nodes"])
    assert r["error"] == 4 and r["stopped"]
    assert r["total_nodes"] - r["nodes"] == 1
