"""The formula kernels on the cases of formula_leaf_cases.py (-m gpu): formfix_kernel (pcp_formula.hip) and setformfix_kernel
(pcp_setform.hip) bit-exact against the oracle — status, rows or sets, and `active` of every node that did not fail — on the exhaustive
Kleene table of every leaf kind, on random stores over every kind with up to 130 units under full, random and single-unit `active` rows
and in batches of 1, 3, 5 and 201 nodes, and on units of exactly 64 and of 67 tree nodes; one tree each of formdfs_kernel and
setformdfs_kernel on three of the random stores.  test_formula_leaf_cpu.py pins what the oracle answers on the same cases."""
import numpy as np
import pytest

from pcp_amd import model as M

import formula_leaf_cases as LC
from test_set_mode import assert_set_parity
from util import assert_parity, random_active

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


def check_plan(ctx, implicit, set_mode):
    pl = ctx.last_plan()
    assert pl["path"] == 3 and pl["set_mode"] == set_mode and pl["implicit_active"] == implicit, pl


def head(ref, n):
    return tuple(a[:n] for a in ref)


def interval_explicit(ctx, L, U, act, ref, what):
    n = L.shape[0]
    got = ctx.propagate(L, U, act[:n])
    check_plan(ctx, 0, 0)
    assert_parity(head(ref, n), got[:4], f"{what} [explicit, {n} nodes]")


def interval_implicit(ctx, L, U, ref, what):
    n = L.shape[0]
    got = ctx.propagate_implicit(L, U)
    check_plan(ctx, 1, 0)
    assert_parity(head(ref, n), got[:4], f"{what} [implicit, {n} nodes]")


def set_explicit(ctx, bits, act, ref, what):
    n = bits.shape[0]
    got = ctx.propagate_set(bits, act[:n])
    check_plan(ctx, 0, 1)
    assert_set_parity(head(ref, n), got[:5], f"{what} [explicit, {n} nodes]")


def set_implicit(ctx, bits, ref, what):
    """Implicit nodes through the device entry, `active` rows materialised on request (as test_setform_gpu.parity does)."""
    import torch
    n, V, _ = bits.shape
    dev = torch.device("cuda", 0)
    t_bits = torch.from_numpy(bits.copy().view(np.int64)).to(dev)
    t_lb = torch.zeros((n, V), dtype=torch.int32, device=dev)
    t_ub = torch.zeros_like(t_lb)
    t_act = torch.zeros((n, max(ctx.words, 1)), dtype=torch.int64, device=dev)
    t_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    ctx.propagate_device(n, None, None, t_lb, t_ub, None, t_act, t_st, 0, bits_in=t_bits, bits_out=t_bits)
    torch.cuda.synchronize()
    check_plan(ctx, 1, 1)
    got = (t_lb.cpu().numpy(), t_ub.cpu().numpy(), t_bits.cpu().numpy().view(np.uint64), t_act.cpu().numpy().view(np.uint64)[:, : ctx.words], t_st.cpu().numpy())
    assert_set_parity(head(ref, n), got, f"{what} [implicit, {n} nodes]")


def push_sets(ctx, vs, cs, sw, base):
    M.push_model(ctx, cs, len(vs), sw)
    ctx.set_hull(base, base + 64 * sw - 1)


# ------------------------------------------------------------------------------------------------------------- (a) Kleene tables
def forms_of(name, tables):
    return [f for n, f in tables if n == name]


@pytest.mark.parametrize("name", LC.VARIANTS)
def test_interval_kleene_table(ctx, name):
    """Every box of the leaf's operands x the guard open, 0 and 1, under each of the table's units: full rows, implicit nodes, and rows with
    the unit switched off in half the nodes (nothing moves there, the status is True)."""
    for form in forms_of(name, LC.INTERVAL_TABLES):
        vs, cs, L, U, _ = LC.interval_table(name, form)
        ref = LC.interval_table_reference(name, form)
        M.push_model(ctx, cs, len(vs))
        assert ctx.n_units == 1
        what = f"table {name} {form}"
        interval_explicit(ctx, L, U, LC.active_rows("full", len(L), 1, 0), ref, what)
        interval_implicit(ctx, L, U, ref, what)
        act = random_active(31, len(L), 1, p_off=0.5)
        interval_explicit(ctx, L, U, act, LC.oracle_model(vs, cs).consistency(L, U, act)[:4], what + " half off")


@pytest.mark.parametrize("sw,base", LC.SET_LAYOUTS)
@pytest.mark.parametrize("name", [n for n in LC.VARIANTS if not LC.VARIANTS[n][3]])
def test_set_kleene_table(ctx, name, sw, base):
    """The set-valued tables: every pair of non-empty subsets (three operands: every box, and the boxes with a hole in x), on one word from
    -2 and on two words with -1 and 0 on either side of the word boundary."""
    for form in forms_of(name, LC.SET_TABLES):
        vs, cs, bits, _ = LC.set_table(name, form, sw, base)
        ref = LC.set_table_reference(name, form, sw, base)
        push_sets(ctx, vs, cs, sw, base)
        assert ctx.n_units == 1
        what = f"set table {name} {form} sw={sw}"
        set_explicit(ctx, bits, LC.active_rows("full", len(bits), 1, 0), ref, what)
        set_implicit(ctx, bits, ref, what)
        act = random_active(32, len(bits), 1, p_off=0.5)
        set_explicit(ctx, bits, act, LC.oracle_model(vs, cs).consistency_set(bits, base, act)[:5], what + " half off")


# ------------------------------------------------------------------------------------------------------------- (b) random stores
@pytest.mark.parametrize("name", LC.RANDOM_CASES)
def test_random_interval_stores(ctx, name):
    """201 nodes under each kind of `active` rows and as implicit nodes; then batches of 1, 3 and 5 nodes (the last workgroup partly empty)
    under full and half-off rows and as implicit nodes."""
    seed = LC.RANDOM_CASES[name][0]
    vs, cs, _, L, U = LC.random_case(name)
    M.push_model(ctx, cs, len(vs))
    assert ctx.n_units == len(cs)
    for kind in LC.ACTIVE_KINDS:
        act = LC.active_rows(kind, len(L), len(cs), seed + 900)
        ref = LC.random_reference(name, kind)
        for n in LC.BATCHES if kind in ("full", "off50") else LC.BATCHES[-1:]:
            interval_explicit(ctx, L[:n], U[:n], act, ref, f"random {name} rows={kind}")
    for n in LC.BATCHES:
        interval_implicit(ctx, L[:n], U[:n], LC.random_reference(name), f"random {name}")


@pytest.mark.parametrize("name", LC.RANDOM_CASES)
def test_random_set_stores(ctx, name):
    seed = LC.RANDOM_CASES[name][0]
    vs, cs, _, bits, sw, base = LC.set_random_case(name)
    push_sets(ctx, vs, cs, sw, base)
    assert ctx.n_units == len(cs)
    for kind in LC.ACTIVE_KINDS:
        act = LC.active_rows(kind, len(bits), len(cs), seed + 950)
        ref = LC.set_random_reference(name, kind)
        for n in LC.BATCHES if kind in ("full", "off50") else LC.BATCHES[-1:]:
            set_explicit(ctx, bits[:n], act, ref, f"random sets {name} rows={kind}")
    for n in LC.BATCHES:
        set_implicit(ctx, bits[:n], LC.set_random_reference(name), f"random sets {name}")


# ------------------------------------------------------------------------------------------------------------- (c) mask edges
def test_units_of_64_and_67_nodes(ctx):
    """An Or of 63 leaves and an And of two Ors (trees of exactly 64 nodes: bit 63 of the masks), next to a Distinct of 66 pairs (the member
    loop) and ordinary units, over intervals and over sets."""
    vs, cs, L, U = LC.mask_edge_case()
    M.push_model(ctx, cs, len(vs))
    ref = LC.mask_edge_reference(False)
    for n in (len(L), 5):
        interval_explicit(ctx, L[:n], U[:n], LC.active_rows("full", len(L), len(cs), 0), ref, "mask edges")
        interval_implicit(ctx, L[:n], U[:n], ref, "mask edges")
    sw, base = LC.MASK_SET_LAYOUT
    bits = M.interval_bits(L, U, sw, base)
    push_sets(ctx, vs, cs, sw, base)
    ref = LC.mask_edge_reference(True)
    for n in (len(L), 5):
        set_explicit(ctx, bits[:n], LC.active_rows("full", len(L), len(cs), 0), ref, "mask edges over sets")
        set_implicit(ctx, bits[:n], ref, "mask edges over sets")


@pytest.mark.parametrize("sw", [0, 1])
def test_a_unit_of_65_nodes_that_is_not_flat_is_refused(ctx, sw):
    """pcp_model_push_formula takes the tree; the lowering, which runs before the first launch, refuses the store (PCP_ERR_UNSUPPORTED):
    the unit step's branch for more than 64 nodes walks a flat Conjunction only."""
    import pcp_amd.engine as E
    vs, cs = LC.not_flat_65()
    M.push_model(ctx, cs, len(vs), sw)
    assert ctx.n_units == 2
    lb0, ub0 = vs.bounds()
    with pytest.raises(E.PcpError) as e:
        if sw:
            ctx.set_hull(-2, 61)
            ctx.propagate_set(M.interval_bits(lb0, ub0, 1, -2)[None], None)
        else:
            ctx.propagate(lb0[None], ub0[None], None)
    assert e.value.code == -5 and "more than 64 nodes" in str(e.value)
    ctx.truncate(1)  # without the unit the store runs
    assert ctx.n_units == 1


# ------------------------------------------------------------------------------------------------------------- forests
@pytest.mark.parametrize("name", LC.FOREST_CASES)
def test_interval_forest_on_the_new_stores(ctx, name):
    """One tree of formdfs_kernel against the oracle's search, 2000 nodes at most: counters and the first solution (test_formula_leaf_cpu
    pins the oracle's counters; below zero the tree is the reference's endless descent, 2000 open rows)."""
    vs, cs, _, _, _ = LC.random_case(name)
    M.push_model(ctx, cs, len(vs))
    lb0, ub0 = vs.bounds()
    ss, _, _, first = LC.oracle_model(vs, cs).search(lb0, ub0, all_solutions=True, node_limit=2000)
    r = ctx.dfs_forest(lb0[None], ub0[None], node_limit_per_tree=2000, steps_per_launch=256, capacity=4096, want_solution=True, formulas=True)
    print("forest", name, (r["nodes"], r["solutions"], r["failed"]), ss)
    assert ctx.last_plan()["path"] == 3 and r["error"] == 0
    assert (r["nodes"], r["solutions"], r["failed"]) == (ss["num_nodes"], ss["num_solution"], ss["num_failed_node"])
    if ss["num_solution"]:
        assert np.array_equal(r["first_solutions"][0], first)


@pytest.mark.parametrize("name", LC.FOREST_CASES)
def test_set_forest_on_the_new_stores(ctx, name):
    """One tree of setformdfs_kernel against the oracle's search over FDSpace, 2000 nodes at most."""
    vs, cs, _, _, sw, base = LC.set_random_case(name)
    push_sets(ctx, vs, cs, sw, base)
    lb0, ub0 = vs.bounds()
    ss, _, _, first = LC.oracle_model(vs, cs).search_set(lb0, ub0, sw, base, all_solutions=True, node_limit=2000)
    # (level_capacity: the driver's default, one level per value of the root, does not hold the endless descent below zero — z34 has 12
    # variables on two words, 1552 levels, and the tree reports error 1 there; 2000 nodes open at most 2000 levels)
    r = ctx.dfs_forest_setform(M.interval_bits(lb0, ub0, sw, base)[None], node_limit=2000, level_capacity=2048)
    print("set forest", name, (r["nodes"], r["solutions"], r["failed"]), ss)
    pl = ctx.last_plan()
    assert pl["path"] == 3 and pl["set_mode"] == 1 and r["error"] == 0
    assert (r["nodes"], r["solutions"], r["failed"]) == (ss["num_nodes"], ss["num_solution"], ss["num_failed_node"])
    if ss["num_solution"]:
        assert np.array_equal(r["first_solution"], first)
