"""The generators of set_wide_cases.py, checked without a GPU: what test_set_wide_gpu.py relies on that is a property of the inputs or of the
reference alone — the statuses each family of fixpoints is meant to reach, the witnesses that a shift mattered, the counts behind the
"more changed variables than the list holds" arguments, the sizes of the reference trees, the mix of statuses of the branching batches.
Conditions on the inputs, fixed before any GPU run; no kernel is measured here."""
import numpy as np
import pytest

from oracle import oracle as orc
from pcp_amd import model as M

import set_wide_cases as W
from test_bnb_forest_cpu import reference_bnb_set_any
from test_bnb_host import reference_bnb_set


@pytest.mark.parametrize("density", list(W.DENSITIES))
@pytest.mark.parametrize("V", W.FIX_VARS)
@pytest.mark.parametrize("sw,base,hi", W.SHAPES)
def test_fixpoint_families_reach_their_statuses(sw, base, hi, V, density):
    assert hi - base + 1 <= 64 * sw and (hi - base + 1 == 64 * sw) == (hi != 290)
    seen = np.zeros(3, np.int64)
    for seed in W.FIX_SEEDS:
        props, bits, act = W.fixpoint_case(sw, base, hi, V, density, seed)
        assert bits.shape == (W.FIX_NODES, V, sw) and bits.any(axis=2).all()
        om = orc.OracleModel(V, props)
        for active in (None, act):  # the implicit and the explicit entry of both_set
            _, _, out, _, st, _ = om.consistency_set(bits, base, active)
            live = st != M.FALSE
            narrowed = (out != bits).any(axis=(1, 2))
            assert 2 * int((narrowed & live).sum()) >= int(live.sum()), (seed, int(narrowed[live].sum()), int(live.sum()))
            if active is None:
                seen += np.bincount(st, minlength=3)[:3]
                if density != "unplanted70":
                    assert (st != M.FALSE).all(), seed  # planted: the hidden solution is in every set
    # the statuses the family is meant to reach, over its seeds
    if density == "planted400":
        assert seen[M.TRUE] > 0, seen  # a long cascade down to the planted values
    elif density == "planted70":
        assert seen[M.UNKNOWN] > 0, seen
    else:
        assert seen[M.FALSE] > 0 and seen[M.UNKNOWN] > 0, seen


@pytest.mark.parametrize("sw", [3, 5])
def test_every_offset_inside_the_universe_has_a_witness_that_the_shift_mattered(sw):
    """XEqY(x, y + d): for every |d| < 64 sw some node's reference result is non-empty and strictly smaller than both inputs."""
    offsets = W.shift_offsets(sw)
    n = 64 * sw
    assert {abs(d) for d in offsets} == {0, 1, 63, 64, 65, 127, 128, n - 1, n, n + 5} and len(offsets) == 19
    for d in offsets:
        bits, (lb, ub, out, act, st) = W.shift_reference("eq", sw, d)
        if abs(d) >= n:
            assert (st == M.FALSE).all(), d  # nothing of y + d is inside the universe
            continue
        size_in, size_out = W.cardinality(bits), W.cardinality(out)
        witness = (st != M.FALSE) & (size_out[:, 0] > 0) & (size_out[:, 0] < size_in[:, 0]) & (size_out[:, 0] < size_in[:, 1])
        assert witness.any(), d
        assert (st == M.FALSE).any(), d  # and a disjoint pair


@pytest.mark.parametrize("sw", [3, 5])
@pytest.mark.parametrize("kind", W.SHIFT_KINDS)
def test_shift_batches_hold_edge_members_and_both_outcomes(kind, sw):
    n, E = 64 * sw, W.edge_positions(sw)
    edge_mask = W.bits_of_positions([E], sw)[0]
    for d in W.shift_offsets(sw):
        for c in (W.shift_constants(sw) if kind.endswith("const") else [None]):
            bits, (lb, ub, out, act, st) = W.shift_reference(kind, sw, d, c)
            assert bits.any(axis=2).all()
            assert ((bits & edge_mask).any(axis=2)).any(axis=1).sum() >= len(bits) - 2  # (all but the purely random rows)
            hit_inside = abs(d) < n - 1 if c is None else 0 <= c + d - W.SHIFT_BASE < n
            if kind.startswith("neq") and hit_inside:
                # a singleton took its value out of the other side in some node, and found it absent in another
                changed = (out != bits).any(axis=(1, 2)) & (st != M.FALSE)
                assert changed.any() and (~changed).any(), (d, c)
            if kind == "neq" and abs(d) >= n:
                assert (st == M.TRUE).all()  # entailed: the shifted sets cannot meet


@pytest.mark.parametrize("variant", range(len(W.STAR_VARIANTS)))
def test_constructed_counts_exceed_the_list(variant):
    # 1. the all-XNeqY star: the hub is the input's only singleton, more than 64 leaves are {a, b}
    V, props, bits, two_valued = W.neq_star(variant)
    a = W.STAR_VARIANTS[variant][0]
    size = W.cardinality(bits)
    assert bits.shape == (W.OVF_NODES, 101, W.OVF_SW) and (props["kind"] == M.NEQ).all() and (props["var"][:, 1] != M.PCP_CONST).all()
    assert (size[:, 0] == 1).all() and (size[:, 1:] >= 2).all()
    holds_a = (bits[:, 1:, a >> 6] >> np.uint64(a & 63)) & np.uint64(1)
    assert (((size[:, 1:] == 2) & (holds_a == 1)).sum(axis=1) == two_valued).all() and (two_valued > W.CAP).all()
    st = orc.OracleModel(V, props).consistency_set(bits, W.OVF_BASE)[4]
    assert (st == M.FALSE).any() and (st != M.FALSE).sum() >= W.OVF_NODES // 2
    # 2. the assigned-variable fallback: more than 64 singletons in the input
    V, props, bits, singles = W.assigned_fallback(variant)
    assert (props["kind"] == M.NEQ).all() and (props["var"][:, 1] != M.PCP_CONST).all()
    assert ((W.cardinality(bits) == 1).sum(axis=1) == singles).all() and (singles > W.CAP).all() and V - int(singles.min()) == 30
    _, _, out, _, st, _ = orc.OracleModel(V, props).consistency_set(bits, W.OVF_BASE)
    assert (st != M.FALSE).any() and ((out != bits).any(axis=(1, 2)) | (st == M.FALSE)).all()
    # 3. the mixed star: not all-XNeqY, more than 64 leaves hold `a` behind a live hub record — with every unit on and with the tests' rows
    V, props, bits, holders = W.mixed_star(variant)
    a = (100, 70, 126)[variant]
    kinds = set(props["kind"].tolist())
    assert M.LT in kinds and M.EQ3 in kinds and M.NEQ in kinds
    assert ((((bits[:, 1:101, a >> 6] >> np.uint64(a & 63)) & np.uint64(1)) == 1) == holders).all()
    assert (W.cardinality(bits)[:, 1:101] == 3).all() and (holders.sum(axis=1) > W.CAP).all()
    om = orc.OracleModel(V, props)
    act = W.mixed_star_active(variant, om.n_units)
    hub_on = ((act[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(W.OVF_NODES, -1)[:, :100] == 1  # unit i - 1 = x0 != x_i
    assert ((holders & hub_on).sum(axis=1) > W.CAP).all()
    for rows in (None, act):
        st = om.consistency_set(bits, W.OVF_BASE, rows)[4]
        assert (st != M.FALSE).sum() >= W.OVF_NODES // 2


def test_the_overflow_csp_is_the_planted_shape_at_three_words():
    V, sw, base, hi, props, bits, act = W.overflow_random_csp()
    assert (V, sw, len(props)) == (91, 3, 400) and V * sw % 2 == 1 and V > W.CAP
    st = orc.OracleModel(V, props).consistency_set(bits, base)[4]
    assert (st == M.TRUE).all()


def _in_range(nodes):
    return 30 <= nodes <= 5000


@pytest.mark.parametrize("brancher,val", W.FOREST_BRANCHERS)
@pytest.mark.parametrize("sw", W.FOREST_SW)
def test_reference_trees_have_30_to_5000_nodes(sw, brancher, val):
    for seed in W.FOREST_SEEDS[(brancher, sw)]:
        V, props, root, base, hull = W.forest_case(sw, brancher, seed)
        size = W.cardinality(root[0])
        assert 6 <= V <= 10 and size.min() >= 3 and size.max() <= 6
        lb, ub = M.bits_bounds(root[0], base)
        assert int(lb.min()) >= (0 if brancher == "split" else base) and int(ub.max()) <= hull[1]
        assert (ub - lb).max() >= 64  # members of one variable in different words
        if brancher == "enumerate":
            assert int(lb.min()) < 0
        assert len(set(props["kind"].tolist())) >= 3 and (props["kind"] >= M.LT3).any()  # a ternary record: rec_at without payloads
        ref = W.forest_reference(sw, brancher, val, seed)
        assert _in_range(ref["nodes"]) and ref["solutions"] > 0, (seed, ref)
        first = W.forest_reference(sw, brancher, val, seed, True)
        assert first["solutions"] == 1 and first["nodes"] <= ref["nodes"]


@pytest.mark.parametrize("brancher,val", W.FOREST_BRANCHERS)
def test_overflow_roots_have_30_to_5000_nodes_below_them(brancher, val):
    for name, (V, props, root) in W.overflow_roots().items():
        assert int(M.bits_bounds(root[0], W.ROOT_BASE)[0].min()) >= 0
        ref = W.tree_reference((name, "root"), V, props, root, W.ROOT_BASE, brancher, val)
        assert _in_range(ref["nodes"]), (name, ref)
    # what makes each root overflow, counted on the root itself
    V, props, root = W.overflow_roots()["neq_star"]
    assert ((W.cardinality(root[0]) == 2).sum() > W.CAP) and (W.cardinality(root[0]) == 1).sum() == 1
    V, props, root = W.overflow_roots()["assigned"]
    assert (W.cardinality(root[0]) == 1).sum() > W.CAP
    V, props, root = W.overflow_roots()["mixed_star"]
    assert (props["kind"] != M.NEQ).any() and (W.cardinality(root[0, 1:101]) >= 3).all()


def test_bnb_reference_trees():
    for brancher in ("split", "enumerate"):
        V, props, lb0, ub0, var, mode, base = W.bnb_case(brancher)
        assert int(lb0.min()) >= 0 and int((ub0 - lb0).max()) == 6
        ref = W.bnb_reference(brancher)
        assert _in_range(ref["nodes"]) and ref["solutions"] >= 1 and ref["failed"] >= 1, ref
        assert lb0[var] <= ref["best"] <= ub0[var]
    # the two restatements agree under BinarySplit
    V, props, lb0, ub0, var, mode, base = W.bnb_case("split")
    a = reference_bnb_set(orc.OracleModel(V, props), lb0, ub0, var, mode == "min", 3, base)
    b = reference_bnb_set_any(orc.OracleModel(V, props), lb0, ub0, var, mode == "min", 3, base)
    assert all(a[k] == b[k] for k in ("nodes", "failed", "solutions", "best"))


@pytest.mark.parametrize("where", W.BRANCH_WHERE)
@pytest.mark.parametrize("sw", [3, 5])
def test_branching_batches_mix_the_statuses(sw, where):
    bits, status, active = W.branch_case(sw, where)
    assert all((status == s).sum() >= 1 for s in (M.FALSE, M.TRUE, M.UNKNOWN))
    size = W.cardinality(bits)
    lb, ub = M.bits_bounds(bits, W.BRANCH_BASE)
    assert int(lb.min()) >= 0
    word = {"first": 0, "middle": sw // 2, "last": sw - 1}[where]
    for i in range(len(bits)):
        key = np.where(size[i] > 1, size[i], 1 << 30)
        var = int(key.argmin())
        assert (key == key[var]).sum() >= 2  # a tie: the first index wins
        others = np.delete(np.arange(sw), word)
        assert bits[i, var, word] != 0 and not bits[i, var, others].any()
