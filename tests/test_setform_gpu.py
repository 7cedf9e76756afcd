"""The reified layer over IntervalSet stores on the GPU (-m gpu): setformfix_kernel (pcp_amd/csrc/pcp_setform.hip, plan.path 3 with
set_mode 1) bit-exact against the oracle's IntervalSet instantiation — sets, bounds, status and `active` — on the random formula stores
test_setform_cpu.py has checked, at the word boundaries of the bit sets, beyond 64 units and beyond 64 tree nodes, on hand-derived
vectors, and under the search drivers."""
import numpy as np
import pytest

from pcp_amd import model as M
from pcp_amd import search as S

import setform_cases as SC
from test_set_mode import assert_set_parity, bits_of, random_sets, values_of
from util import random_active

pytestmark = pytest.mark.gpu

BATCHES = (1, 5, 67)  # one node; a workgroup whose last wavefront slots stay empty; more nodes than one generation of one workgroup


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


def push(ctx, vs, cs, sw, hull):
    M.push_model(ctx, cs, len(vs), sw)
    ctx.set_hull(*hull)


def check_plan(ctx, implicit):
    pl = ctx.last_plan()
    assert pl["path"] == 3 and pl["set_mode"] == 1 and pl["implicit_active"] == implicit, pl


def parity(ctx, vs, cs, bits, base, hull, what, batches=BATCHES, active_seed=None):
    """Implicit nodes (rows materialised on request) and explicit random rows, each at every batch size, against the oracle."""
    import torch
    om = SC.oracle_model(vs, cs)
    sw, V, n_all = bits.shape[2], len(vs), bits.shape[0]
    push(ctx, vs, cs, sw, hull)
    assert ctx.n_units == om.n_units == len(cs)
    ref_i = om.consistency_set(bits, base, None)[:5]
    act = random_active(active_seed if active_seed is not None else 77, n_all, om.n_units, p_off=0.15)
    ref_e = om.consistency_set(bits, base, act)[:5]
    dev = torch.device("cuda", 0)
    for n in batches:
        assert n <= n_all
        got = ctx.propagate_set(bits[:n], act[:n])
        check_plan(ctx, 0)
        assert_set_parity(tuple(a[:n] for a in ref_e), got[:5], f"{what} [explicit, {n} nodes]")
        t_bits = torch.from_numpy(bits[:n].copy().view(np.int64)).to(dev)
        t_lb = torch.zeros((n, V), dtype=torch.int32, device=dev)
        t_ub = torch.zeros_like(t_lb)
        t_act = torch.zeros((n, max(ctx.words, 1)), dtype=torch.int64, device=dev)
        t_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        ctx.propagate_device(n, None, None, t_lb, t_ub, None, t_act, t_st, 0, bits_in=t_bits, bits_out=t_bits)
        torch.cuda.synchronize()
        check_plan(ctx, 1)
        got_i = (t_lb.cpu().numpy(), t_ub.cpu().numpy(), t_bits.cpu().numpy().view(np.uint64), t_act.cpu().numpy().view(np.uint64)[:, : ctx.words], t_st.cpu().numpy())
        assert_set_parity(tuple(a[:n] for a in ref_i), got_i, f"{what} [implicit, {n} nodes]")
    return ref_i, ref_e


@pytest.mark.parametrize("seed", SC.SEEDS)
def test_random_formula_stores_over_sets(ctx, seed):
    """The 40 stores of test_setform_cpu.py (12 variables, about 10 units), 67 random set-valued nodes each (the first 8 are the CPU file's)."""
    vs, cs, bits = SC.random_case(seed, n_nodes=67)
    assert np.array_equal(bits[:8], SC.random_case(seed)[2])
    parity(ctx, vs, cs, bits, 0, (0, 6), f"set formula store seed={seed}", active_seed=2000 + seed)


@pytest.mark.parametrize("sw,base", [(3, -66), (1, -3)])
@pytest.mark.parametrize("seed", range(6))
def test_word_boundaries(ctx, seed, sw, base):
    """dom = (-3, 3).  With 3 words from -66, value -3 is bit 63 of word 0 and -2 is bit 0 of word 1; with one word from -3 the domain
    starts at bit 0."""
    vs, cs, bits = SC.random_case(seed, dom=(-3, 3), sw=sw, base=base, n_nodes=16)
    if sw == 3:
        assert (bits[:, :, 0] >> np.uint64(63)).any() and (bits[:, :, 1] & np.uint64(1)).any()
    ref_i, _ = parity(ctx, vs, cs, bits, base, (base, base + 64 * sw - 1), f"word boundary sw={sw} seed={seed}", batches=(16,), active_seed=3000 + seed)
    assert len(ref_i[4]) == 16


@pytest.mark.parametrize("seed", [500, 506])
def test_more_than_64_units(ctx, seed):
    """70 units: lanes take a second unit each (the lane-strided pass), and `active` rows are two words wide."""
    vs, cs, bits = SC.wide_case(seed)
    assert len(cs) == 70
    ref_i, ref_e = parity(ctx, vs, cs, bits, 0, (0, 6), f"70 units seed={seed}", batches=(24,), active_seed=seed + 1)
    for ref in (ref_i, ref_e):
        ok = ref[4] != 0
        assert ok.sum() >= 8 and (ref[3][ok, 1] != 0).any() and (ref[2][ok] != bits[ok]).any()  # open nodes that narrowed, units past 64 live


def test_unit_of_more_than_64_nodes(ctx):
    """Distinct over 12 variables next to an equivalence: 66 pairs = a flat Conjunction of 67 tree nodes, walked by the member loop."""
    vs, cs = M.VStore(), M.CStore()
    xs = [vs.alloc((0, 13)) for _ in range(12)]
    b = vs.alloc((0, 1))
    cs.alloc(M.Distinct(xs))
    cs.alloc(M.equivalence(M.Boolean(b), M.XLessY(xs[0], xs[1])))
    lb, ub = vs.bounds()
    bits = random_sets(611, lb, ub, 24, 1, 0, p_keep=0.8)
    bits[:8, :3] = M.interval_bits(np.array([3, 5, 7]), np.array([3, 5, 7]), 1, 0)  # assigned variables: the Distinct removes their values
    ref_i, _ = parity(ctx, vs, cs, bits, 0, (0, 13), "Distinct(12) + equivalence", batches=(24,), active_seed=612)
    assert (ref_i[4] != 0).any() and (ref_i[2][ref_i[4] != 0] != bits[ref_i[4] != 0]).any()


def test_hand_vectors(ctx):
    vs, cs, bits = SC.hand_or_eq_bool()
    push(ctx, vs, cs, 1, (0, 63))
    lb, ub, out, act, st, _ = ctx.propagate_set(bits, np.ones((1, 1), np.uint64))
    check_plan(ctx, 0)
    assert st[0] == M.TRUE and int(act[0, 0]) == 0
    assert [values_of(w) for w in out[0]] == [[1, 3, 5], [2, 4], [1]]
    assert (lb[0].tolist(), ub[0].tolist()) == ([1, 2, 1], [5, 4, 1])
    vs, cs, bits = SC.hand_implication()
    push(ctx, vs, cs, 1, (0, 63))
    lb, ub, out, act, st, _ = ctx.propagate_set(bits, np.ones((1, 1), np.uint64))
    assert [values_of(w) for w in out[0]] == [[2], [1, 3], [3, 4, 5]]
    assert st[0] == M.TRUE and int(act[0, 0]) == 0 and (lb[0, 2], ub[0, 2]) == (3, 5)


def test_boolean_on_a_set_without_one_fails_the_node(ctx):
    """A top-level Boolean(b) with b = {0}: Boolean::propagate would be a non-monotonic update, the reference panics
    (variable/store.rs:153-156); the engine fails the node (contract difference vi)."""
    vs, cs = M.VStore(), M.CStore()
    b = vs.alloc((0, 1))
    cs.alloc(M.Boolean(b))
    push(ctx, vs, cs, 1, (0, 63))
    st = ctx.propagate_set(np.stack([bits_of([0])])[None], None)[4]
    check_plan(ctx, 1)
    assert st[0] == M.FALSE
    out = ctx.propagate_set(np.stack([bits_of([0, 1])])[None], None)  # ... and with 1 in the set it is assigned
    assert out[4][0] == M.TRUE and values_of(out[2][0, 0]) == [1]


def test_fixpoints_are_idempotent(ctx):
    """The output rows of one parity batch propagated again: nothing changes, the statuses are equal."""
    vs, cs, bits = SC.random_case(3, n_nodes=67)
    push(ctx, vs, cs, 1, (0, 6))
    act = random_active(2003, 67, len(cs), p_off=0.15)
    lb, ub, out, act1, st, _ = ctx.propagate_set(bits, act)
    ok = st != M.FALSE
    assert ok.any() and (out[ok] != bits[ok]).any()
    lb2, ub2, out2, act2, st2, stats = ctx.propagate_set(out[ok], act1[ok])
    assert np.array_equal(st2, st[ok]) and np.array_equal(out2, out[ok]) and np.array_equal(act2, act1[ok])
    assert np.array_equal(lb2, lb[ok]) and np.array_equal(ub2, ub[ok]) and stats["narrowings"] == 0


DUR = (2, 3, 2, 1)


def schedule_is_valid(sol):
    s = [int(v) for v in sol[:4]]
    pairs = all(s[i] + DUR[i] <= s[j] or s[j] + DUR[j] <= s[i] for i in range(4) for j in range(i + 1, 4))
    return pairs and (int(sol[4]) == 1) == (s[0] < s[2])


def test_search_over_a_disjunctive_schedule(ctx):
    """All solutions of a four-task disjunctive schedule through search.dfs_set and DeviceSearch == the oracle's DFS over FDSpace; the
    device branchers read sets, status and unit rows only."""
    from pcp_amd.search_device import DeviceSearch
    vs, cs, _, _ = SC.disjunctive_schedule(DUR, 8)
    V = len(vs)
    lb0, ub0 = vs.bounds()
    ss, _, _, _ = SC.oracle_model(vs, cs).search_set(lb0, ub0, 1, 0, all_solutions=True)
    assert ss["num_solution"] > 0 and ss["num_failed_node"] > 0
    want = (ss["num_solution"], ss["num_nodes"], ss["num_failed_node"])
    push(ctx, vs, cs, 1, (0, 63))
    for implicit in (True, False):
        st = S.dfs_set(ctx, lb0, ub0, 0, all_solutions=True, implicit=implicit)
        check_plan(ctx, int(implicit))
        assert (st.num_solution, st.num_nodes, st.num_failed_node) == want
        assert len(st.solutions) == want[0] and all(schedule_is_valid(s) for s in st.solutions)
        for brancher in ("split", "enumerate") if implicit else ("split",):  # (the Enumerate driver takes implicit nodes only)
            ds = DeviceSearch(ctx, batch=1 if brancher == "split" else 16, capacity=1024, implicit=implicit, brancher=brancher)
            dv = ds.run(lb0, ub0, all_solutions=True, keep_solutions=64, base=0)
            assert dv.num_solution == want[0] and len({tuple(s) for s in dv.solutions}) == want[0]
            assert all(schedule_is_valid(s) for s in dv.solutions)
            if brancher == "split":
                assert (dv.num_nodes, dv.num_failed_node) == want[1:]
    en = S.dfs_enumerate_set(ctx, lb0, ub0, 0, all_solutions=True)
    assert en.num_solution == want[0] and all(schedule_is_valid(s) for s in en.solutions)


def test_what_stays_refused(ctx):
    import pcp_amd.engine as E
    vs, cs, _, _ = SC.disjunctive_schedule(DUR, 8)
    push(ctx, vs, cs, 1, (0, 63))
    root = M.interval_bits(*vs.bounds(), 1, 0)[None]
    with pytest.raises(E.PcpError) as e:  # the forest's kernel evaluates records, not trees
        ctx.dfs_forest_set(root)
    assert e.value.code == -5 and "formula" in str(e.value)
    V = 4
    mul = M.lower_units([M.XEqYMulZ(M.Identity(0), M.Identity(1), M.Identity(2))], V)
    sums = []
    sum_leaf = M.lower_units([M.XLessY(M.Sum((M.Identity(0), M.Identity(1))), M.Identity(2))], V, sums_out=sums)
    nodes = np.zeros(3, dtype=M.FNODE_DTYPE)
    nodes[0] = (M.F_OR, 0, 2, 1); nodes[1] = (M.F_LEAF, 0, 0, 0); nodes[2] = (M.F_LEAF, 0, 0, 1)
    boolean = M.lower_units([M.Boolean(M.Identity(3))], V)
    for leaf in (mul, sum_leaf):
        ctx.reset_model(V, 1)
        ctx.push_sum(sums[0])
        with pytest.raises(E.PcpError) as e:  # as a prop
            ctx.push_props(leaf)
        assert e.value.code == -5
        with pytest.raises(E.PcpError) as e:  # as a formula leaf
            ctx.push_formula(nodes, np.concatenate([boolean, leaf]))
        assert e.value.code == -5
        assert ctx.n_units == 0
        ctx.push_formula(nodes, np.concatenate([boolean, M.lower_units([M.XLessY(M.Identity(0), M.Identity(2))], V)]))
        assert ctx.n_units == 1
