"""Enumerate over IntervalSet stores on the device (DESIGN.md §2 "Value selection on a set"):
  * pcp_branch_device_set_enum, bit for bit against pcp_amd.search.branch_enumerate_set;
  * pcp_dfs_forest_device_set_enum: one tree rooted at the root IS the left-first DFS under Brancher<FirstSmallestVar, MiddleVal | MinVal,
    Enumerate> (the judge of enum_set_ref.py: one oracle call per node), launch length by launch length; a forest below a frontier adds up to
    the same tree, with and without pcp_dfs_forest_split_set;
  * DeviceSearch(brancher="enumerate") over a set-mode context and search_forest.forest_search_set(brancher="enumerate");
  * the BinarySplit loop still is the oracle's search_set."""
import numpy as np
import pytest

from oracle import oracle as orc
from pcp_amd import model as M
from pcp_amd import search as S

from enum_set_ref import SET_KINDS, nqueens_model, nqueens_tree, reference_dfs
from util import random_csp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    return E.Context(0)


def _unit_model(ctx, V, sw, base):
    """A set-mode model of V variables whose hull is all of set_words words from `base` (the brancher reads no propagator: V units x != base)."""
    p = np.zeros(V, dtype=M.PROP_DTYPE)
    p["kind"] = M.NEQ
    p["var"][:] = [0, M.PCP_CONST, M.PCP_NOVAR]
    p["var"][:, 0] = np.arange(V)
    p["off"][:, 1] = base
    p["group"] = np.arange(V)
    ctx.set_model(V, p, set_words=sw)
    ctx.set_hull(base, base + 64 * sw - 1)


def _rows_of(sets, sw, base):
    """bits [n, V, sw], lb, ub [n, V] from sets[node][var] = the values."""
    n, V = len(sets), len(sets[0])
    bits = np.zeros((n, V, sw), np.uint64)
    lb, ub = np.zeros((n, V), np.int32), np.zeros((n, V), np.int32)
    for i, row in enumerate(sets):
        for j, vals in enumerate(row):
            for v in vals:
                k, bit = divmod(int(v) - base, 64)
                bits[i, j, k] |= np.uint64(1) << np.uint64(bit)
            lb[i, j], ub[i, j] = min(vals), max(vals)
    return bits, lb, ub


def _branch_on_device(ctx, bits, lb, ub, status, val, active=None, reverse=False):
    """One call of pcp_branch_device_set_enum: (child bits [k, V, sw], child active or None, counts[8])."""
    import torch
    dev = torch.device("cuda", ctx.device)
    n, V, sw = bits.shape
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
    child = torch.full((2 * n, V, sw), 0x5A5A5A5A, dtype=torch.int64, device=dev)
    cact = None if active is None else torch.zeros((2 * n, active.shape[1]), dtype=torch.int64, device=dev)
    counts = torch.full((8,), 7, dtype=torch.int32, device=dev)
    ctx.set_option("branch_reverse", int(reverse))
    try:
        ctx.branch_device_set_enum(n, t(bits, np.int64), t(lb, np.int32), t(ub, np.int32), None if active is None else t(active, np.int64), t(status, np.uint8), val,
                                   child, cact, counts, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
    finally:
        ctx.set_option("branch_reverse", 0)
    c = counts.cpu().numpy()
    k = int(c[0])
    return child.cpu().numpy().view(np.uint64)[:k], (None if cact is None else cact.cpu().numpy().view(np.uint64)[:k]), c


def _check_against_the_host_brancher(ctx, bits, lb, ub, status, base, val, active, reverse):
    unk = status == M.UNKNOWN
    want_b, want_a = S.branch_enumerate_set(bits[unk], lb[unk], ub[unk], base, None if active is None else active[unk], val=val)
    if reverse:
        want_b, want_a = want_b[::-1], (None if want_a is None else want_a[::-1])
    got_b, got_a, c = _branch_on_device(ctx, bits, lb, ub, status, val, active, reverse)
    assert c.tolist() == [2 * int(unk.sum()), int((status == M.TRUE).sum()), int((status == M.FALSE).sum()), int(unk.sum()), int((status > M.UNKNOWN).sum()), 0, 0, 0]
    assert np.array_equal(got_b, want_b), (val, reverse)
    if active is not None:
        assert np.array_equal(got_a, want_a)


@pytest.mark.parametrize("sw", [1, 2, 3])
@pytest.mark.parametrize("V", [1, 5, 70, 257])
def test_brancher_kernel_is_the_host_brancher(ctx, V, sw):
    for base in (1, -70):
        _unit_model(ctx, V, sw, base)
        words = (ctx.n_units + 63) // 64
        rng = np.random.default_rng(1000 * V + 10 * sw + (base < 0))
        for n in (1, 3, 65):
            # random sets with holes: one to six values anywhere in the hull, so that cardinalities tie and minima sit at any index
            sets = [[sorted(set(int(x) for x in rng.integers(base, base + 64 * sw, size=int(rng.integers(1, 7))))) for _ in range(V)] for _ in range(n)]
            status = rng.choice(np.array([M.FALSE, M.TRUE, M.UNKNOWN, M.UNKNOWN, 3], np.uint8), size=n)
            status[0] = M.UNKNOWN
            for i in np.nonzero(status == M.UNKNOWN)[0]:  # an Unknown node has a variable to branch on
                j = int(rng.integers(0, V))
                if not any(len(s) > 1 for s in sets[i]):
                    sets[i][j] = sorted({base, base + 64 * sw - 1, *sets[i][j]})
            bits, lb, ub = _rows_of(sets, sw, base)
            active = rng.integers(0, 1 << 62, size=(n, words)).astype(np.uint64)
            for val in ("middle", "min"):
                for reverse in (False, True):
                    for act in (None, active):
                        _check_against_the_host_brancher(ctx, bits, lb, ub, status, base, val, act, reverse)


@pytest.mark.parametrize("base", [1, -70])
def test_brancher_kernel_targeted_rows(ctx, base):
    """Holes at m, v at bits 0, 63 and 64, the nearest member in another word on either side and two words away, ties, a negative sum."""
    V, sw = 3, 5
    _unit_model(ctx, V, sw, base)
    b = base
    rows = [
        [b + 1, b + 2, b + 3, b + 4, b + 5],       # m a member
        [b, b + 1, b + 7, b + 8],                  # m a hole, a tie: the lower member
        [b, b + 3, b + 7, b + 8],                  # the nearer member below
        [b, b + 1, b + 6, b + 8],                  # the nearer member above
        [b, b + 1],                                # v at bit 0
        [b + 63, b + 64],                          # m = bit 63
        [b + 64, b + 66],                          # m a hole at bit 65: bit 64 (bit 0 of word 1)
        [b + 62, b + 63, b + 64],                  # MinVal at bit 62, MiddleVal at bit 63
        [b, b + 60, b + 70, b + 130],              # m in word 1, a tie with a member of word 0
        [b, b + 59, b + 70, b + 130],              # ... the nearer member in word 1
        [b, b + 3, b + 300],                       # m in word 2, words 1 and 2 empty: two words below
        [b, b + 297, b + 300],                     # two words above
        [b + 319, b],                              # the whole hull's ends
        [b + 5, b + 6, b + 64 * sw - 1],
    ]
    others = [[b + 17], [b + 200]]  # singletons: variable 1 is the only one to branch on
    sets = [[others[0], r, others[1]] for r in rows]
    bits, lb, ub = _rows_of(sets, sw, base)
    status = np.full(len(rows), M.UNKNOWN, np.uint8)
    for val in ("middle", "min"):
        for reverse in (False, True):
            _check_against_the_host_brancher(ctx, bits, lb, ub, status, base, val, None, reverse)
    # and the values themselves, by the rule as DESIGN states it (not through the host brancher)
    got_b, _, _ = _branch_on_device(ctx, bits, lb, ub, status, "middle")
    for i, r in enumerate(rows):
        s = min(r) + max(r)
        m = abs(s) // 2 * (1 if s >= 0 else -1)
        v = min(r, key=lambda c: (abs(c - m), c > m))
        assert S.set_members(got_b[2 * i, 1], base).tolist() == [v], (i, r, m)
        assert S.set_members(got_b[2 * i + 1, 1], base).tolist() == sorted(c for c in r if c != v)


def test_brancher_contract(ctx):
    import torch
    import pcp_amd.engine as E
    dev = torch.device("cuda", ctx.device)
    V, sw, base = 5, 2, 1
    _unit_model(ctx, V, sw, base)
    sets = [[[3]] * V, [[2, 9]] + [[4]] * (V - 1)]
    bits, lb, ub = _rows_of(sets, sw, base)
    # n_nodes = 0: PCP_OK, all eight counts zeroed
    counts = torch.full((8,), 7, dtype=torch.int32, device=dev)
    ctx.branch_device_set_enum(0, None, None, None, None, None, "min", None, None, counts, 0)
    torch.cuda.synchronize(dev)
    assert counts.cpu().tolist() == [0] * 8
    # error 3: an Unknown node whose variables are all assigned; the counts of the scan are still those of the batch
    _, _, c = _branch_on_device(ctx, bits, lb, ub, np.array([M.UNKNOWN, M.UNKNOWN], np.uint8), "middle")
    assert c.tolist() == [4, 0, 0, 2, 0, 0, 3, 0]
    # val out of range, a null required pointer
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
    args = [t(bits, np.int64), t(lb, np.int32), t(ub, np.int32), None, t(np.array([2, 2], np.uint8), np.uint8)]
    child = torch.zeros((4, V, sw), dtype=torch.int64, device=dev)
    with pytest.raises(E.PcpError) as e:
        ctx.branch_device_set_enum(2, *args, 2, child, None, counts, 0)
    assert e.value.code == -1
    with pytest.raises(E.PcpError) as e:
        ctx.branch_device_set_enum(2, None, *args[1:], "min", child, None, counts, 0)
    assert e.value.code == -1
    with pytest.raises(E.PcpError) as e:
        ctx.branch_device_set_enum(2, *args, "min", child, None, None, 0)
    assert e.value.code == -1
    # an interval-mode model
    ctx.set_model(6, M.nqueens_props(6))
    with pytest.raises(E.PcpError) as e:
        ctx.branch_device_set_enum(2, *args, "min", child, None, counts, 0)
    assert e.value.code == -5
    torch.cuda.synchronize(dev)


def nqueens(ctx, n):
    props, sw, lb0, ub0 = nqueens_model(n)
    ctx.set_model(n, props, set_words=sw)
    ctx.set_hull(1, n)
    return props, sw, lb0, ub0


def root_bits(lb0, ub0, sw, base):
    return M.interval_bits(np.asarray(lb0), np.asarray(ub0), sw, base)[None]


def _counters(r):
    return {k: r[k] for k in ("nodes", "solutions", "failed")}


def _tree(ref):
    return {k: ref[k] for k in ("nodes", "solutions", "failed")}


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("n,steps", [(6, 1), (6, 7), (6, 2048), (7, 1), (7, 7), (7, 2048), (8, 1), (8, 7), (8, 2048), (9, 7), (9, 2048)])
def test_one_tree_is_the_reference_dfs(ctx, n, steps, val):
    """steps = 1: every launch ends between a node and its right child."""
    props, sw, lb0, ub0 = nqueens(ctx, n)
    ref = nqueens_tree(n, val)
    r = ctx.dfs_forest_set(root_bits(lb0, ub0, sw, 1), steps_per_launch=steps, brancher="enumerate", val=val)
    assert r["error"] == 0 and r["finished_trees"] == 1
    assert _counters(r) == _tree(ref) and r["total_nodes"] == r["nodes"]
    first = nqueens_tree(n, val, first_only=True)
    one = ctx.dfs_forest_set(root_bits(lb0, ub0, sw, 1), stop_on_solution=True, steps_per_launch=steps, brancher="enumerate", val=val)
    assert one["stopped"] and one["solutions"] == 1
    assert one["nodes"] == first["nodes"] and one["failed"] == first["failed"]
    assert np.array_equal(one["first_solution"], first["first"])


def test_a_wide_hull_uses_several_words(ctx):
    """n = 70: two words per set, to the first solution under MinVal."""
    n = 70
    props, sw, lb0, ub0 = nqueens(ctx, n)
    assert sw == 2
    first = nqueens_tree(n, "min", first_only=True)
    one = ctx.dfs_forest_set(root_bits(lb0, ub0, sw, 1), stop_on_solution=True, steps_per_launch=50, brancher="enumerate", val="min")
    assert one["error"] == 0 and one["solutions"] == 1
    assert one["nodes"] == first["nodes"] and one["failed"] == first["failed"]
    assert np.array_equal(one["first_solution"], first["first"])


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("seed", range(8))
def test_mixed_kinds_one_tree(ctx, seed, val):
    """The random CSPs of test_set_forest.test_mixed_kinds_one_tree, over every propagator kind set mode has."""
    rng = np.random.default_rng(7100 + seed)
    V = int(rng.integers(5, 9))
    hi = int(rng.integers(4, 8))
    props, _, _, _ = random_csp(7200 + seed, V, int(rng.integers(6, 14)), planted=bool(seed & 1), dom=(0, hi), kinds=SET_KINDS)
    lb0, ub0 = np.zeros(V, np.int32), np.full(V, hi, np.int32)
    ref = reference_dfs(("mixed", seed), V, props, M.interval_bits(lb0, ub0, 1, 0), 0, val)
    ctx.set_model(V, props, set_words=1)
    ctx.set_hull(0, hi)
    r = ctx.dfs_forest_set(root_bits(lb0, ub0, 1, 0), steps_per_launch=int(rng.integers(3, 40)), brancher="enumerate", val=val)
    assert r["error"] == 0
    assert _counters(r) == _tree(ref), (seed, val)


@pytest.mark.parametrize("val", ["middle", "min"])
def test_node_limit_is_exact_and_the_search_resumes(ctx, val):
    n, K = 9, 57
    props, sw, lb0, ub0 = nqueens(ctx, n)
    assert nqueens_tree(n, val)["nodes"] > K
    ref = nqueens_tree(n, val, node_limit=K)
    r = ctx.dfs_forest_set(root_bits(lb0, ub0, sw, 1), node_limit=K, steps_per_launch=16, brancher="enumerate", val=val)
    assert r["stopped"] and r["nodes"] == K and r["total_nodes"] == K and r["finished_trees"] == 0
    assert (r["solutions"], r["failed"]) == (ref["solutions"], ref["failed"])


def test_a_full_trail_is_reported(ctx):
    n = 8
    props, sw, lb0, ub0 = nqueens(ctx, n)
    r = ctx.dfs_forest_set(root_bits(lb0, ub0, sw, 1), trail_capacity=8, steps_per_launch=64, brancher="enumerate", val="middle")
    assert r["error"] == 4 and r["stopped"]


def _frontier(ctx, lb0, ub0, rounds, val):
    from pcp_amd.search_device import DeviceSearch
    ds = DeviceSearch(ctx, batch=4096, capacity=8192, implicit=True, brancher="enumerate", val=val)
    ds.reset(lb0, ub0, 1)
    for _ in range(rounds):  # breadth-first: every open node of a level in one round
        if ds.advance(all_solutions=True, max_rounds=1, keep_solutions=0):
            break
    ds.compact()
    return ds.bits[:ds.size].clone(), ds.stats


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("n,rounds,steps", [(8, 3, 5), (9, 4, 6)])
def test_forest_below_a_frontier_with_and_without_splits(ctx, n, rounds, steps, val):
    """Few trees of very different sizes (an Enumerate frontier is lopsided: {v} against the rest) and short launches: finished trees take
    over the oldest open right branch of the others (pcp_dfs_forest_split_set reads the distributor from the level); expansion + forest is
    the one Enumerate tree either way."""
    props, sw, lb0, ub0 = nqueens(ctx, n)
    ref = nqueens_tree(n, val)
    roots, st = _frontier(ctx, lb0, ub0, rounds, val)
    assert roots.shape[0] > 1
    want = {"nodes": ref["nodes"] - st.num_nodes, "solutions": ref["solutions"] - st.num_solution, "failed": ref["failed"] - st.num_failed_node}
    info = {}
    r = ctx.dfs_forest_set(roots, steps_per_launch=steps, info=info, brancher="enumerate", val=val)
    assert r["error"] == 0 and _counters(r) == want and r["finished_trees"] == roots.shape[0]
    assert info["splits"] > 0  # `done` was non-zero at least once
    plain = ctx.dfs_forest_set(roots, steps_per_launch=steps, rebalance=False, brancher="enumerate", val=val)
    assert plain["error"] == 0 and _counters(plain) == want and plain["splits"] == 0


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("n", [6, 7, 8])
def test_device_search_enumerate_in_set_mode(ctx, n, val):
    from pcp_amd.search_device import DeviceSearch
    props, sw, lb0, ub0 = nqueens(ctx, n)
    ref = nqueens_tree(n, val)
    assert ctx.supports_set_enumerate
    for batch in (1, 5, 64):
        ds = DeviceSearch(ctx, batch=batch, implicit=True, brancher="enumerate", val=val)
        st = ds.run(lb0, ub0, all_solutions=True, keep_solutions=1 << 20, base=1)
        got = {"nodes": st.num_nodes, "solutions": st.num_solution, "failed": st.num_failed_node}
        assert got == _tree(ref), (batch, got)
        assert sorted(tuple(int(x) for x in s) for s in st.solutions) == ref["sols"]


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("n,trees", [(8, 4), (9, 16)])
def test_forest_search_driver_single_and_two_ranks(ctx, n, trees, val):
    from pcp_amd.search_forest import forest_search_set
    props, sw, lb0, ub0 = nqueens(ctx, n)
    want = _tree(nqueens_tree(n, val))
    one = forest_search_set(ctx, lb0, ub0, 1, n_trees=trees, steps_per_launch=32, brancher="enumerate", val=val)
    assert one["error"] == 0 and _counters(one) == want
    parts = [forest_search_set(ctx, lb0, ub0, 1, n_trees=trees, steps_per_launch=32, rank=r, world=2, brancher="enumerate", val=val) for r in range(2)]
    assert all(p["error"] == 0 for p in parts) and all(p["trees"] > 0 for p in parts)
    assert {k: sum(p[k] for p in parts) for k in want} == want


def test_binary_split_is_untouched(ctx):
    """dfs_forest_set() without the new arguments is still the oracle's search_set (the kernel gained a template parameter)."""
    n = 8
    props, sw, lb0, ub0 = nqueens(ctx, n)
    ss, _, _, sol1 = orc.OracleModel(n, props).search_set(lb0, ub0, sw, 1, all_solutions=True)
    for steps in (1, 7, 2048):
        r = ctx.dfs_forest_set(root_bits(lb0, ub0, sw, 1), steps_per_launch=steps)
        assert r["error"] == 0 and (r["solutions"], r["nodes"], r["failed"]) == (ss["num_solution"], ss["num_nodes"], ss["num_failed_node"])
    ss1, _, _, sol1 = orc.OracleModel(n, props).search_set(lb0, ub0, sw, 1)
    one = ctx.dfs_forest_set(root_bits(lb0, ub0, sw, 1), stop_on_solution=True, steps_per_launch=7)
    assert one["nodes"] == ss1["num_nodes"] and np.array_equal(one["first_solution"], sol1)
