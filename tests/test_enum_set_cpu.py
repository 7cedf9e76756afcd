"""Enumerate over IntervalSet stores, the parts that need no GPU (DESIGN.md §2 "Value selection on a set"):
  * folding x = v / x != v into the variable's set is what the reference's XEqY(x, Constant v) / XNeqY(x, Constant v) do on an IntervalSet;
  * pcp_amd.search.branch_enumerate_set against the table of enumerate.rs:71-77 and the value rule case by case;
  * search.dfs_enumerate_set and DeviceSearch(brancher="enumerate") over oracle-backed set contexts against a plain DFS loop."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as orc
from pcp_amd import model as M
from pcp_amd import search as S
import pcp_amd.engine as E
from pcp_amd.search_device import DeviceSearch

from enum_set_ref import SET_KINDS, SetOracleCtx, SetOracleDeviceCtx, nqueens_model, nqueens_tree, reference_dfs
from util import random_csp


def _bits_of(sets, sw, base):
    """[V, sw] uint64 from one list of values per variable."""
    b = np.zeros((len(sets), sw), np.uint64)
    for i, vals in enumerate(sets):
        for v in vals:
            k, bit = divmod(int(v) - base, 64)
            b[i, k] |= np.uint64(1) << np.uint64(bit)
    return b


def _unit(kind, x, v, group):
    """x == Constant(v) or x != Constant(v) as one more propagator behind the model's (Branch::distribute, branch.rs:36-55)."""
    p = np.zeros(1, dtype=M.PROP_DTYPE)
    p["kind"] = kind
    p["var"][:] = [x, M.PCP_CONST, M.PCP_NOVAR]
    p["off"][:, 1] = v
    p["group"] = group
    return p


def test_abi_lists_the_entries():
    for name in ("pcp_branch_device_set_enum", "pcp_dfs_forest_device_set_enum"):
        assert name in E.ABI_SYMBOLS  # (tests/test_abi.py then checks the header and the export)
        assert name in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "integration", "pcp-hip-sys", "src", "lib.rs")).read()


@pytest.mark.parametrize("seed", range(12))
def test_folding_is_the_reference_propagator(seed):
    """consistency_set on the model plus XEqY(x, Constant v) from the parent's sets == consistency_set on the model from the child with the
    set of x folded to {v}; the same for XNeqY(x, Constant v) and the cleared bit.  Values within one word and within two, negative base."""
    rng = np.random.default_rng(9100 + seed)
    V = int(rng.integers(3, 9))
    two_words = bool(seed & 1)
    base = int(rng.integers(-70, -2)) if seed % 3 else int(rng.integers(0, 3))
    span = int(rng.integers(66, 100)) if two_words else int(rng.integers(4, 12))
    sw = 2 if two_words else 1
    lo, hi = base, base + span - 1
    props, _, _, _ = random_csp(9200 + seed, V, int(rng.integers(4, 12)), planted=bool(seed & 2), dom=(lo, hi), kinds=SET_KINDS)
    om = orc.OracleModel(V, props)
    # the parent: random sets with holes, every variable keeps at least one value and one variable at least two
    sets = [sorted(set(int(x) for x in rng.choice(np.arange(lo, hi + 1), size=int(rng.integers(1, min(span, 9) + 1)), replace=False))) for _ in range(V)]
    x = int(rng.integers(0, V))
    if len(sets[x]) < 2:
        sets[x] = sorted({lo, hi, *sets[x]})
    parent = _bits_of(sets, sw, base)
    v = int(rng.choice(sets[x]))
    k, bit = divmod(v - base, 64)
    one = np.uint64(1) << np.uint64(bit)
    left, right = parent.copy(), parent.copy()
    left[x] = 0
    left[x, k] = one
    right[x, k] &= ~one
    group = int(props["group"].max()) + 1
    for kind, child in ((M.EQ, left), (M.NEQ, right)):
        ref = orc.OracleModel(V, np.concatenate([props, _unit(kind, x, v, group)])).consistency_set(parent[None], base)
        got = om.consistency_set(child[None], base)
        assert ref[4][0] == got[4][0], (seed, kind)
        if ref[4][0] != M.FALSE:
            assert np.array_equal(ref[2], got[2]) and np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1]), (seed, kind)


def test_branch_enumerate_set_against_the_reference_table(golden_dir):
    kats = json.load(open(os.path.join(golden_dir, "enumerate_kats.json")))
    assert len(kats["distribution"]) == 3
    for row in kats["distribution"]:
        lb, ub = (np.array(c, np.int32) for c in zip(*row["root"]))
        bits = M.interval_bits(lb, ub, 1, 1)
        B, A = S.branch_enumerate_set(bits[None], lb[None], ub[None], 1, None, val=row["val"], var=row["var"])
        assert A is None and B.shape == (2, len(lb), 1)
        for child, (clo, chi) in zip(B, row["children"]):
            want = bits.copy()
            want[row["var"]] = M.interval_bits(np.array([clo]), np.array([chi]), 1, 1)[0]
            assert np.array_equal(child, want), row["source"]
    # read as sets: {1} / 2..10, {2} / 3..4, {1} / {2}
    got = [[S.set_members(B_[r["var"]], 1).tolist() for B_ in S.branch_enumerate_set(M.interval_bits(*(np.array(c, np.int32) for c in zip(*r["root"])), 1, 1)[None],
                                                                                      *(np.array(c, np.int32)[None] for c in zip(*r["root"])), 1, None, val="min", var=r["var"])[0]]
           for r in kats["distribution"]]
    assert got == [[[1], list(range(2, 11))], [[2], [3, 4]], [[1], [2]]]
    assert len(kats["impossible"]) == 2
    for row in kats["impossible"]:
        lb, ub = (np.array(c, np.int32) for c in zip(*row["root"]))
        with pytest.raises(RuntimeError, match="Cannot select a variable"):
            S.branch_enumerate_set(M.interval_bits(lb, ub, 1, 1)[None], lb[None], ub[None], 1, None, val=row["val"], var=row["var"])


# (values of the set, base, set_words) -> MiddleVal's value, computed by hand
VALUE_RULE = [
    ((1, 2, 3, 4, 5), 1, 1, 3),            # m = 3 is a member: the reference's value
    ((1, 2, 4, 5, 9), 1, 1, 5),            # m = 5 is a member of a set with holes
    ((1, 2, 8, 9), 1, 1, 2),               # m = 5 a hole, members at distance 3 on both sides: the lower one wins
    ((1, 4, 8, 9), 1, 1, 4),               # m = 5 a hole, the nearer member below
    ((1, 2, 7, 9), 1, 1, 7),               # m = 5 a hole, the nearer member above
    ((0, 60, 70, 130), 0, 3, 60),          # m = 65 in word 1; 60 (word 0) and 70 are as near: the lower one, in another word
    ((0, 59, 70, 130), 0, 3, 70),          # ... 70 is nearer
    ((0, 66, 130), 0, 3, 66),              # m = 65 a hole, the member next to it
    ((0, 3, 300), 0, 5, 3),                # m = 150 in word 2, which is empty like word 1: the nearest member two words below
    ((0, 297, 300), 0, 5, 297),            # ... two words above
    ((-7, -6, -2, 0), -7, 1, -2),          # lower + upper = -7: m = -3, truncated toward zero (floor -4 would tie and take -6)
    ((-70, -9, -8, -3), -70, 2, -9),       # m = -73 / 2 = -36: a hole, -9 the nearest
    ((-5, -4, -1, 0), -70, 2, -1),         # lower + upper = -5: m = -2 (floor -3 would take -4)
    ((63, 64), 0, 2, 63),                  # m = 63: bit 63 of word 0
    ((64, 66), 0, 2, 64),                  # m = 65 a hole: 64 (bit 0 of word 1) before 66
]


@pytest.mark.parametrize("values,base,sw,want", VALUE_RULE)
def test_the_value_rule(values, base, sw, want):
    bits = _bits_of([values], sw, base)[0]
    lo, hi = min(values), max(values)
    s = lo + hi
    m = abs(s) // 2 * (1 if s >= 0 else -1)
    assert want == min(values, key=lambda c: (abs(c - m), c > m))  # (the table is consistent with the rule as DESIGN states it)
    got = S.enumerate_value_set(bits, lo, hi, base, "middle")
    assert got == want, (values, m, got)
    if m in values:
        assert got == m  # exactly the reference (middle_val.rs:25-27)
    assert S.enumerate_value_set(bits, lo, hi, base, "min") == lo  # MinVal: lower(), always a member
    # and through the brancher: {v} / the set without v
    B, _ = S.branch_enumerate_set(bits[None, None], np.array([[lo]]), np.array([[hi]]), base, None, val="middle")
    assert S.set_members(B[0, 0], base).tolist() == [got] and S.set_members(B[1, 0], base).tolist() == [c for c in sorted(values) if c != got]


def _stats(st):
    return {"nodes": st.num_nodes, "solutions": st.num_solution, "failed": st.num_failed_node, "sols": sorted(tuple(int(x) for x in s) for s in st.solutions)}


def _same_tree(got, ref):
    return all(got[k] == ref[k] for k in ("nodes", "solutions", "failed", "sols"))


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("n", [5, 6, 7, 8])
def test_dfs_enumerate_set_on_the_oracle_context(n, val):
    props, sw, lb0, ub0 = nqueens_model(n)
    ref = nqueens_tree(n, val)
    # an independent check: the BinarySplit tree of the oracle has the same solutions
    ss, _, _, _ = orc.OracleModel(n, props).search_set(lb0, ub0, sw, 1, all_solutions=True)
    assert ref["solutions"] == ss["num_solution"] == len(set(ref["sols"]))
    split = S.dfs_set(SetOracleCtx(n, props, sw, 1), lb0, ub0, 1, all_solutions=True)
    assert sorted(tuple(int(x) for x in s) for s in split.solutions) == ref["sols"]
    for batch in (1, 4):
        got = _stats(S.dfs_enumerate_set(SetOracleCtx(n, props, sw, 1), lb0, ub0, 1, all_solutions=True, batch=batch, val=val))
        assert _same_tree(got, ref), (batch, got["nodes"], ref["nodes"])
    # one solution: the reference's first
    one = S.dfs_enumerate_set(SetOracleCtx(n, props, sw, 1), lb0, ub0, 1, val=val)
    first = nqueens_tree(n, val, first_only=True)
    assert one.num_solution == 1 and one.num_nodes == first["nodes"] and np.array_equal(one.solutions[0], first["first"])


@pytest.mark.parametrize("val", ["middle", "min"])
def test_dfs_enumerate_set_obeys_stop_node(val):
    n = 6
    props, sw, lb0, ub0 = nqueens_model(n)
    size = nqueens_tree(n, val)["nodes"]
    assert size > 20
    for limit in list(range(1, 12)) + [size - 1, size]:
        ref = nqueens_tree(n, val, node_limit=limit)
        got = _stats(S.dfs_enumerate_set(SetOracleCtx(n, props, sw, 1), lb0, ub0, 1, all_solutions=True, node_limit=limit, val=val))
        assert _same_tree(got, ref) and got["nodes"] == limit, (limit, got, ref)


@pytest.mark.parametrize("val", ["middle", "min"])
@pytest.mark.parametrize("n", [5, 6, 7])
def test_device_search_over_a_stand_in_that_offers_the_set_brancher(n, val):
    import torch
    props, sw, lb0, ub0 = nqueens_model(n)
    want = _stats(S.dfs_enumerate_set(SetOracleCtx(n, props, sw, 1), lb0, ub0, 1, all_solutions=True, val=val))
    assert _same_tree(want, nqueens_tree(n, val))
    for batch in (1, 5, 64):
        ctx = SetOracleDeviceCtx(n, props, sw, 1)
        ds = DeviceSearch(ctx, batch=batch, device=torch.device("cpu"), implicit=True, brancher="enumerate", val=val)
        assert type(ds.kind).__name__ == "_SetsEnumerate" and ds.dirty is None and not hasattr(ds, "ex")  # no hints, no arena
        st = ds.run(lb0, ub0, all_solutions=True, keep_solutions=1 << 20, base=1)
        assert _same_tree(_stats(st), want), (batch, st.num_nodes, want["nodes"])
        assert ctx.branch_calls == st.rounds and not ds.segs


def test_device_search_refuses_a_set_context_without_the_entry():
    import torch
    n = 6
    props, sw, lb0, ub0 = nqueens_model(n)
    ctx = SetOracleDeviceCtx(n, props, sw, 1)
    ctx.supports_set_enumerate = False
    with pytest.raises(ValueError, match=r"set mode.*pcp_branch_device_set_enum"):
        DeviceSearch(ctx, batch=4, device=torch.device("cpu"), implicit=True, brancher="enumerate")
    ctx.supports_set_enumerate = True
    kw = dict(batch=4, device=torch.device("cpu"), brancher="enumerate")
    with pytest.raises(ValueError, match="cells"):
        DeviceSearch(ctx, implicit=True, cells=True, **kw)
    with pytest.raises(ValueError, match="objective"):
        DeviceSearch(ctx, implicit=True, objective=(0, "min"), **kw)
    with pytest.raises(ValueError, match="implicit"):
        DeviceSearch(ctx, implicit=False, **kw)


def test_mixed_kinds_reference_tree_has_the_solutions_of_the_split_tree():
    """The judge itself on random mixed-kind CSPs: Enumerate and BinarySplit enumerate the same solutions."""
    for seed in range(4):
        rng = np.random.default_rng(7100 + seed)
        V, hi = int(rng.integers(5, 9)), int(rng.integers(4, 8))
        props, _, _, _ = random_csp(7200 + seed, V, int(rng.integers(6, 14)), planted=bool(seed & 1), dom=(0, hi), kinds=SET_KINDS)
        lb0, ub0 = np.zeros(V, np.int32), np.full(V, hi, np.int32)
        ss, _, _, _ = orc.OracleModel(V, props).search_set(lb0, ub0, 1, 0, all_solutions=True)
        for val in ("middle", "min"):
            ref = reference_dfs(("mixed", seed), V, props, M.interval_bits(lb0, ub0, 1, 0), 0, val)
            assert ref["solutions"] == ss["num_solution"]
