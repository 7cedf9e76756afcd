"""Set-mode kernels (pcp_set.hip) beyond two words per set and past the changed-variable list, bit-exact against the CPU oracle, which keeps an
IntervalSet as a list of intervals and shares no bit arithmetic with the kernels:
  1. setfix_kernel / set_derive_active_kernel at 3, 5 and 8 words, rows of even and odd length (V * set_words odd: the scalar staging path, every
     second row misaligned), through the three entries of test_set_mode.both_set;
  2. window / intersect_shifted / disjoint_shifted / clear_range at word edges: x ◇ y + d for offsets around 64, 128 and the universe's size;
  3. list_cap = 64: the `total > C` sweep of setfix_kernel on an all-XNeqY and on a mixed model, and the `ns > C` fallback;
  4. setdfs_kernel (all four instantiations) on sparse roots of 3 and 5 words, and below roots that overflow the list;
  5. set_branch_kernel at 3 and 5 words.
The cases and their references come from set_wide_cases.py; what they promise about themselves is asserted in test_set_wide_cpu.py."""
import numpy as np
import pytest

from oracle import oracle as orc
from pcp_amd import model as M
from pcp_amd import search as S

import set_wide_cases as W
from test_set_mode import assert_set_parity, both_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import pcp_amd.engine as E
    c = E.Context(0)
    yield c
    c.close()


class list_cap:
    """ctx.set_option("list_cap", n) for a block, 2048 (the default) afterwards."""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n

    def __enter__(self):
        self.ctx.set_option("list_cap", self.n)

    def __exit__(self, *exc):
        self.ctx.set_option("list_cap", 2048)


# ------------------------------------------------------------------------------------------- 1. fixpoints at 3, 5 and 8 words
@pytest.mark.parametrize("density", list(W.DENSITIES))
@pytest.mark.parametrize("V", W.FIX_VARS)
@pytest.mark.parametrize("sw,base,hi", W.SHAPES)
def test_fixpoint_parity_on_wide_sets(ctx, sw, base, hi, V, density):
    if V == 91 and sw % 2:
        assert V * sw % 2 == 1
    for seed in W.FIX_SEEDS:
        props, bits, act = W.fixpoint_case(sw, base, hi, V, density, seed)
        both_set(ctx, V, props, bits, base, (base, hi), act, f"wide csp sw={sw} hi={hi} V={V} {density} seed={seed}")
        assert ctx.last_plan()["list_cap"] == 1024  # (the default: the list holds every variable here)


# ------------------------------------------------------------------------------------------- 2. shifts at word edges
@pytest.mark.parametrize("sw", [3, 5])
@pytest.mark.parametrize("kind", W.SHIFT_KINDS)
def test_shifts_at_word_edges(ctx, kind, sw):
    hull = (W.SHIFT_BASE, W.SHIFT_BASE + 64 * sw - 1)
    for d in W.shift_offsets(sw):
        for c in (W.shift_constants(sw) if kind.endswith("const") else [None]):
            V, props = W.shift_model(kind, d, c)
            bits, ref = W.shift_reference(kind, sw, d, c)
            got_ref, _ = both_set(ctx, V, props, bits, W.SHIFT_BASE, hull, None, f"shift {kind} sw={sw} d={d} c={c}")
            assert np.array_equal(got_ref[4], ref[4])  # (both_set's own reference is the shared one)


# ------------------------------------------------------------------------------------------- 3. more changed variables than the list holds
def _implicit(ctx, V, props, bits, base, what):
    """Implicit nodes through the host entry: the fixpoint against the oracle; returns the plan of the launch."""
    sw = bits.shape[2]
    ctx.set_model(V, props, set_words=sw)
    ctx.set_hull(base, base + 64 * sw - 1)
    ref = orc.OracleModel(V, props).consistency_set(bits, base, None)
    got = ctx.propagate_set(bits, None)
    pl = ctx.last_plan()
    assert pl["set_mode"] == 1 and pl["implicit_active"] == 1
    assert_set_parity(ref[:5], (got[0], got[1], got[2], None, got[4]), what, check_active=False)
    return pl


@pytest.mark.parametrize("variant", range(len(W.STAR_VARIANTS)))
def test_neq_star_overflows_the_list(ctx, variant):
    """total > C on an all-XNeqY model: round 0 lists 70 or more new singletons (set_wide_cases.neq_star)."""
    V, props, bits, _ = W.neq_star(variant)
    with list_cap(ctx, W.CAP):
        assert _implicit(ctx, V, props, bits, W.OVF_BASE, f"neq star {variant}")["list_cap"] == W.CAP
        both_set(ctx, V, props, bits, W.OVF_BASE, (W.OVF_BASE, W.OVF_BASE + 64 * W.OVF_SW - 1), None, f"neq star {variant}")
        assert ctx.last_plan()["list_cap"] == W.CAP


@pytest.mark.parametrize("variant", range(len(W.STAR_VARIANTS)))
def test_assigned_variable_fallback(ctx, variant):
    """ns > C: 70 singletons in the input of an all-XNeqY model; the same nodes with the default capacity take the assigned-variable sweep."""
    V, props, bits, _ = W.assigned_fallback(variant)
    with list_cap(ctx, W.CAP):
        assert _implicit(ctx, V, props, bits, W.OVF_BASE, f"assigned fallback {variant} cap 64")["list_cap"] == W.CAP
        both_set(ctx, V, props, bits, W.OVF_BASE, (W.OVF_BASE, W.OVF_BASE + 64 * W.OVF_SW - 1), None, f"assigned fallback {variant} cap 64")
    assert _implicit(ctx, V, props, bits, W.OVF_BASE, f"assigned fallback {variant} cap 2048")["list_cap"] == 1024


@pytest.mark.parametrize("variant", range(len(W.STAR_VARIANTS)))
def test_mixed_star_overflows_the_list(ctx, variant):
    """total > C on a model that is not all-XNeqY: explicit `active` rows (some units off), every unit on, implicit nodes."""
    V, props, bits, _ = W.mixed_star(variant)
    hull = (W.OVF_BASE, W.OVF_BASE + 64 * W.OVF_SW - 1)
    with list_cap(ctx, W.CAP):
        ctx.set_model(V, props, set_words=W.OVF_SW)
        act = W.mixed_star_active(variant, ctx.n_units)
        both_set(ctx, V, props, bits, W.OVF_BASE, hull, act, f"mixed star {variant} [rows]")
        assert ctx.last_plan()["list_cap"] == W.CAP
        both_set(ctx, V, props, bits, W.OVF_BASE, hull, None, f"mixed star {variant} [all on]")


def test_random_csp_with_a_short_list(ctx):
    V, sw, base, hi, props, bits, act = W.overflow_random_csp()
    assert V * sw % 2 == 1
    with list_cap(ctx, W.CAP):
        both_set(ctx, V, props, bits, base, (base, hi), act, "planted csp, list_cap 64")
        assert ctx.last_plan()["list_cap"] == W.CAP


# ------------------------------------------------------------------------------------------- 4. the forest kernel on wide sets
def _one_tree(ctx, V, props, root, base, hull, brancher, val, ref, first, what):
    ctx.set_model(V, props, set_words=root.shape[2])
    ctx.set_hull(*hull)
    for steps in W.FOREST_STEPS:
        r = ctx.dfs_forest_set(root, steps_per_launch=steps, brancher=brancher, val=val)
        print(what, steps, "device", (r["solutions"], r["nodes"], r["failed"]), "reference", (ref["solutions"], ref["nodes"], ref["failed"]))
        assert r["error"] == 0 and r["finished_trees"] == 1 and r["total_nodes"] == r["nodes"]
        assert (r["solutions"], r["nodes"], r["failed"]) == (ref["solutions"], ref["nodes"], ref["failed"]), (what, steps)
        assert r["launches"] >= -(-ref["nodes"] // steps)
        one = ctx.dfs_forest_set(root, stop_on_solution=True, steps_per_launch=steps, brancher=brancher, val=val)
        assert one["error"] == 0 and one["stopped"] and one["solutions"] == 1
        assert (one["nodes"], one["failed"]) == (first["nodes"], first["failed"]), (what, steps)
        assert np.array_equal(one["first_solution"], first["first"])


@pytest.mark.parametrize("brancher,val", W.FOREST_BRANCHERS)
@pytest.mark.parametrize("sw", W.FOREST_SW)
def test_one_tree_on_sparse_wide_roots(ctx, sw, brancher, val):
    for seed in W.FOREST_SEEDS[(brancher, sw)]:
        V, props, root, base, hull = W.forest_case(sw, brancher, seed)
        _one_tree(ctx, V, props, root, base, hull, brancher, val, W.forest_reference(sw, brancher, val, seed), W.forest_reference(sw, brancher, val, seed, True),
                  f"tree sw={sw} {brancher}/{val} seed={seed}")


@pytest.mark.parametrize("brancher,val", W.FOREST_BRANCHERS)
@pytest.mark.parametrize("name", ["neq_star", "assigned", "mixed_star"])
def test_one_tree_below_a_root_that_overflows_the_list(ctx, name, brancher, val):
    """list_cap = 64 inside setdfs_kernel: the root's round 0 lists more than 64 variables (neq_star, mixed_star) or its sweep meets more than 64
    assigned variables (assigned)."""
    V, props, root = W.overflow_roots()[name]
    hull = (W.ROOT_BASE, W.ROOT_BASE + 64 * W.OVF_SW - 1)
    ref = W.tree_reference((name, "root"), V, props, root, W.ROOT_BASE, brancher, val)
    first = W.tree_reference((name, "root"), V, props, root, W.ROOT_BASE, brancher, val, first_only=True)
    with list_cap(ctx, W.CAP):
        _one_tree(ctx, V, props, root, W.ROOT_BASE, hull, brancher, val, ref, first, f"root {name} {brancher}/{val}")
        assert ctx.last_plan()["list_cap"] == W.CAP


@pytest.mark.parametrize("brancher", ["split", "enumerate"])
def test_branch_and_bound_at_three_words(ctx, brancher):
    V, props, lb0, ub0, var, mode, base = W.bnb_case(brancher)
    ref = W.bnb_reference(brancher)
    ctx.set_model(V, props, set_words=3)
    ctx.set_hull(base, base + 191)
    root = M.interval_bits(lb0, ub0, 3, base)[None]
    for steps in W.FOREST_STEPS:
        r = ctx.dfs_forest_set_bnb(root, (var, mode), steps_per_launch=steps, brancher=brancher)
        print(brancher, steps, "device", (r["nodes"], r["failed"], r["solutions"], r["best"]), "reference", (ref["nodes"], ref["failed"], ref["solutions"], ref["best"]))
        assert r["error"] == 0 and r["finished_trees"] == 1 and not r["stopped"]
        assert (r["nodes"], r["failed"], r["solutions"], r["best"]) == (ref["nodes"], ref["failed"], ref["solutions"], ref["best"])
        row = r["best_solution"]
        assert row is not None and int(row[var]) == ref["best"]
        assert int(orc.OracleModel(V, props).consistency_set(M.interval_bits(row, row, 3, base)[None], base)[4][0]) == M.TRUE


# ------------------------------------------------------------------------------------------- 5. BinarySplit branching on wide sets
def _unit_model(ctx, V, sw, base):
    """A set-mode model of V variables and V units over the whole universe (the brancher reads no propagator)."""
    p = np.zeros(V, dtype=M.PROP_DTYPE)
    p["kind"] = M.NEQ
    p["var"][:] = [0, M.PCP_CONST, M.PCP_NOVAR]
    p["var"][:, 0] = np.arange(V)
    p["off"][:, 1] = base
    p["group"] = np.arange(V)
    ctx.set_model(V, p, set_words=sw)
    ctx.set_hull(base, base + 64 * sw - 1)


@pytest.mark.parametrize("where", W.BRANCH_WHERE)
@pytest.mark.parametrize("sw", [3, 5])
def test_binary_split_brancher_on_wide_sets(ctx, sw, where):
    import torch
    dev = torch.device("cuda", ctx.device)
    bits, status, active = W.branch_case(sw, where)
    n, V, _ = bits.shape
    _unit_model(ctx, V, sw, W.BRANCH_BASE)
    assert ctx.words == active.shape[1]
    lb, ub = M.bits_bounds(bits, W.BRANCH_BASE)
    unk = status == M.UNKNOWN
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
    for act in (None, active):
        want_b, want_a = S.branch_set(bits[unk], lb[unk], ub[unk], W.BRANCH_BASE, None if act is None else act[unk])
        for reverse in (0, 1):
            child = torch.full((2 * n, V, sw), 0x5A5A5A5A, dtype=torch.int64, device=dev)
            cact = None if act is None else torch.zeros((2 * n, act.shape[1]), dtype=torch.int64, device=dev)
            counts = torch.full((8,), 7, dtype=torch.int32, device=dev)
            ctx.set_option("branch_reverse", reverse)
            try:
                ctx.branch_device_set(n, t(bits, np.int64), t(lb, np.int32), t(ub, np.int32), None if act is None else t(act, np.int64), t(status, np.uint8),
                                      child, cact, counts, torch.cuda.current_stream(dev).cuda_stream)
                torch.cuda.synchronize(dev)
            finally:
                ctx.set_option("branch_reverse", 0)
            c = counts.cpu().numpy()
            k = 2 * int(unk.sum())
            assert c[:5].tolist() == [k, int((status == M.TRUE).sum()), int((status == M.FALSE).sum()), int(unk.sum()), 0]
            got_b = child.cpu().numpy().view(np.uint64)[:k]
            assert np.array_equal(got_b, want_b[::-1] if reverse else want_b), (sw, where, reverse)
            if act is not None:
                got_a = cact.cpu().numpy().view(np.uint64)[:k]
                assert np.array_equal(got_a, want_a[::-1] if reverse else want_a)
