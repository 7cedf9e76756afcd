"""smallfix_kernel (pcp_small.hip, one wavefront per node, plan.path 4) on the cases of small_cases.py (-m gpu), bit-exact against the
oracle — status of every node; rows and `active` of every node that did not fail — at the edges of its 128-value all-different mask, of
its unit lanes and tables, of its staging words and of its node loop, and with node units on a store that has a grouped Distinct.
test_small_cases_cpu.py proves that the cases reach those edges.

Every case runs through the device entry (the host entry refuses a row with lb > ub, which the node loop's cases hold) under explicit
`active` rows and as implicit nodes; a case with a Distinct once more with small_alldiff = 0, the unit pair by pair: same answer (the
step counters differ, the mask needs fewer rounds).  After every launch the plan says which kernel ran: path 4, and for the two stores
beyond the path's limits (129 slots, 2049 records) any other."""
import numpy as np
import pytest

from pcp_amd import model as M

import small_cases as SC
from util import assert_parity

pytestmark = pytest.mark.gpu

OPTIONS = {"force_path": 0, "nodes_per_block": 0, "block_threads": 1024, "team": 0, "list_cap": 2048, "global_dom": 0, "packed": 1, "word_level": 1,
           "group_level": 1, "small_path": 1, "small_alldiff": 1, "neq_path": 1}


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    for k, v in OPTIONS.items():
        c.set_option(k, v)
    yield c
    c.close()


def launch(ctx, L, U, act, small=True, node_units=None):
    """One launch through pcp_propagate_device (pcp_propagate_device_units with node_units = (offsets, rows)); act None: implicit nodes.
    Returns (lb, ub, active, status, stats, plan)."""
    import torch
    n = L.shape[0]
    dev = torch.device("cuda", ctx.device)
    t_lb, t_ub = torch.from_numpy(np.array(L, np.int32, order="C")).to(dev), torch.from_numpy(np.array(U, np.int32, order="C")).to(dev)
    t_in = None if act is None else torch.from_numpy(np.array(act, np.uint64, order="C").view(np.int64)).to(dev)
    t_out = torch.full((n, max(ctx.words, 1)), -1, dtype=torch.int64, device=dev)
    t_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    before = ctx.stats_read(stream)
    if act is None:
        ctx.set_option("neq_path", 0)  # (a store of XNeqY alone would take pcp_neq.hip as implicit nodes)
    try:
        if node_units is None:
            ctx.propagate_device(n, t_lb, t_ub, t_lb, t_ub, t_in, t_out, t_st, stream)
        else:
            off, rows = node_units
            ctx.propagate_device_units(n, t_lb, t_ub, t_lb, t_ub, t_in, t_out, t_st, torch.from_numpy(off).to(dev),
                                       torch.from_numpy(rows.view(np.uint8).copy()).to(dev), stream)
    finally:
        ctx.set_option("neq_path", 1)
    plan = ctx.last_plan()
    assert (plan["path"] == 4) == small and plan["implicit_active"] == (1 if act is None else 0), plan
    after = ctx.stats_read(stream)
    out = t_out.cpu().numpy().view(np.uint64)[:, : ctx.words]
    # no bit of `active_out` at or above the unit count, on failed nodes neither (assert_parity does not compare their rows): every launch,
    # explicit rows and implicit nodes (where the staging's tail mask alone clears them), grouped and pair by pair
    assert out.shape == (n, (ctx.n_units + 63) // 64) and tail_is_clear(out, ctx.n_units), (plan, ctx.n_units)
    return t_lb.cpu().numpy(), t_ub.cpu().numpy(), out, t_st.cpu().numpy(), {k: after[k] - before[k] for k in after}, plan


def tail_is_clear(act, n_units):
    return n_units % 64 == 0 or not (act[:, -1] >> np.uint64(n_units % 64)).any()


def head(ref, n):
    return tuple(a[:n] for a in ref)


def check_case(ctx, key, batches=(None,)):
    """The case under its own `active` rows (None: every unit) and as implicit nodes, in batches of its first n nodes; with a Distinct,
    the same again pair by pair.  Returns the results of the last batch under explicit rows."""
    import pcp_amd.engine as E
    name, n_vars, props, L, U, act, _ = SC.CASES[key]()
    small = key not in SC.LIMIT_CASES
    ctx.set_model(n_vars, props)
    rows = act if act is not None else E.full_active(len(L), ctx.n_units)
    ref, ref_i = SC.reference(key), SC.implicit_reference(key)
    for n in batches:
        n = n or len(L)
        got = launch(ctx, L[:n], U[:n], rows[:n], small)
        assert_parity(head(ref, n), got[:4], f"{name} [explicit, {n} nodes]")
        got_i = launch(ctx, L[:n], U[:n], None, small)
        assert_parity(head(ref_i, n), got_i[:4], f"{name} [implicit, {n} nodes]")
        if key in SC.DISTINCT_CASES + ("C",):
            ctx.set_option("small_alldiff", 0)
            try:
                pair, pair_i = launch(ctx, L[:n], U[:n], rows[:n], small), launch(ctx, L[:n], U[:n], None, small)
            finally:
                ctx.set_option("small_alldiff", 1)
            assert_parity(head(ref, n), pair[:4], f"{name} [explicit, pair by pair, {n} nodes]")
            assert_parity(head(ref_i, n), pair_i[:4], f"{name} [implicit, pair by pair, {n} nodes]")
            assert_parity(got[:4], pair[:4], f"{name} [grouped against pair by pair, {n} nodes]")
            assert_parity(got_i[:4], pair_i[:4], f"{name} [implicit, grouped against pair by pair, {n} nodes]")
    return got


# ---------------------------------------------------------------------------------------------------------------- A the mask, the lanes
@pytest.mark.parametrize("key", SC.DISTINCT_CASES)
def test_all_different_mask_and_lane_edges(ctx, key):
    """A1: hulls of 126 .. 129 values from -130 .. 5, runs across the mask's word boundaries, duplicates at bits 0, 64 and 127.  A2: a hull
    of 200 that comes under the mask after the first round.  A3: units of 3, 63 and 64 variables (2016 pair records).  A4: nine Distinct
    units behind 31 or 63 others (ids on 31 | 32 and 63 | 64), the ninth pair by pair, rows that switch single ones off."""
    check_case(ctx, key, batches=(None, 5))


# ---------------------------------------------------------------------------------------------------------------- B staging
@pytest.mark.parametrize("key", [f"B-S{s}" for s in SC.B_SLOTS] + [f"B-U{u}" for u in SC.B_UNITS])
def test_staging_words_and_lanes(ctx, key):
    """Stores of exactly 63 .. 128 slots and of exactly 1 .. 129 units, in batches of 1, 3, 4, 5 and 101 nodes; no bit of `active_out` at
    or above the unit count, on failed nodes neither (launch() asserts it after every launch)."""
    check_case(ctx, key, batches=SC.B_BATCHES)


@pytest.mark.parametrize("key", SC.LIMIT_CASES)
def test_one_step_beyond_the_limits_takes_another_kernel(ctx, key):
    """129 slots, or 2049 records: not this kernel (launch() asserts path != 4), and the oracle's answer all the same."""
    check_case(ctx, key, batches=(None, 3))


# ---------------------------------------------------------------------------------------------------------------- C the node loop
def test_a_wavefront_takes_several_nodes(ctx):
    """12288 rows of the 64-variable store — more than the grid's wavefronts, so each takes a second and a third node and finds the LDS slice
    (fail and refusal flags, changed mask, live and entailed words) as the node before left it.  The rows repeat with period 127, which the
    stride does not divide: a wavefront's consecutive nodes differ, True, False (duplicates, lb > ub on input) and Unknown in turn."""
    import pcp_amd.engine as E
    _, n_vars, props, L0, U0, _, _ = SC.c_case()
    ref = tuple(SC.c_expand(a) for a in SC.reference("C"))
    L, U = SC.c_expand(L0), SC.c_expand(U0)
    N = SC.C_NODES
    n_failed = int((ref[3] == M.FALSE).sum())
    ctx.set_model(n_vars, props)
    rows = E.full_active(N, ctx.n_units)
    for alldiff in (1, 0):
        ctx.set_option("small_alldiff", alldiff)
        try:
            for act in (rows, None):
                got = launch(ctx, L, U, act)
                plan, stats = got[5], got[4]
                stride = plan["grid"] * plan["block"] // 64
                assert stride < N and stride % SC.C_PERIOD != 0, plan
                assert_parity(ref, got[:4], f"node loop alldiff={alldiff} implicit={act is None}")
                assert stats["nodes"] == N and stats["failed_nodes"] == n_failed, stats
        finally:
            ctx.set_option("small_alldiff", 1)


# ---------------------------------------------------------------------------------------------------------------- D node units
def test_node_units_on_a_store_with_a_grouped_distinct(ctx):
    """N-queens 8 with one Distinct: nodes with 0, 1, 63, 64, 65 and 70 propagators of their own (the lane-strided loop's second trip),
    each against the oracle over the model plus that node's propagators; implicit nodes and explicit rows, grouped and pair by pair."""
    import pcp_amd.engine as E
    (_, n_vars, props, L, U, _, _), units = SC.d_case()
    ref = SC.d_reference()
    off = np.zeros(len(L) + 1, np.int32)
    off[1:] = np.cumsum([len(u) for u in units])
    flat = np.concatenate(units)
    ctx.set_model(n_vars, props)
    rows = E.full_active(len(L), ctx.n_units)
    ok = ref[3] != M.FALSE
    for alldiff in (1, 0):
        ctx.set_option("small_alldiff", alldiff)
        try:
            for act in (None, rows):
                lb, ub, _, st, _, _ = launch(ctx, L, U, act, node_units=(off, flat))
                what = f"node units alldiff={alldiff} implicit={act is None}"
                assert np.array_equal(st, ref[3]), (what, np.nonzero(st != ref[3])[0][:10])
                assert np.array_equal(lb[ok], ref[0][ok]) and np.array_equal(ub[ok], ref[1][ok]), what
        finally:
            ctx.set_option("small_alldiff", 1)
