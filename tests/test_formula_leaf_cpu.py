"""The cases of formula_leaf_cases.py, specification side (no GPU): what the oracle answers on them, pinned, so that the GPU file
(test_formula_leaf_gpu.py) cannot pass vacuously — every Kleene table has nodes where the leaf is entailed, disentailed and undecided
under an open guard, and nodes the leaf's filter narrows and fails under a closed one; every random case has its share of nodes whose
rows are compared, a node that ends True, and every leaf kind in its lowered tables; the mask-edge nodes do what they were built for."""
import numpy as np
import pytest

from pcp_amd import model as M

import formula_leaf_cases as LC

# (guard open: True, guard assigned, unchanged | guard closed: operands narrowed, failed) — the oracle's figures (table_counts)
INTERVAL_COUNTS = {
    ("NEQ-1", "or_g"): (89, 4, 221, 32, 4), ("NEQ-1", "or_not_g"): (89, 4, 221, 32, 4), ("NEQ-1", "equiv"): (89, 89, 136, 162, 89),
    ("EQ-1", "or_g"): (89, 85, 140, 130, 85), ("EQ-1", "or_not_g"): (89, 85, 140, 130, 85), ("EQ-1", "equiv"): (89, 89, 136, 162, 89),
    ("LT-1", "or_g"): (129, 114, 111, 91, 114), ("LT-1", "or_not_g"): (129, 114, 111, 91, 114), ("LT-1", "equiv"): (129, 129, 96, 146, 129),
    ("NEQ+0", "or_g"): (75, 5, 220, 40, 5), ("NEQ+0", "or_not_g"): (75, 5, 220, 40, 5), ("NEQ+0", "equiv"): (75, 75, 150, 180, 75),
    ("EQ+0", "or_g"): (75, 70, 155, 140, 70), ("EQ+0", "or_not_g"): (75, 70, 155, 140, 70), ("EQ+0", "equiv"): (75, 75, 150, 180, 75),
    ("LT+0", "or_g"): (105, 70, 155, 105, 70), ("LT+0", "or_not_g"): (105, 70, 155, 105, 70), ("LT+0", "equiv"): (105, 105, 120, 190, 105),
    ("NEQ+2", "or_g"): (122, 3, 222, 24, 3), ("NEQ+2", "or_not_g"): (122, 3, 222, 24, 3), ("NEQ+2", "equiv"): (122, 122, 103, 124, 122),
    ("EQ+2", "or_g"): (122, 119, 106, 100, 119), ("EQ+2", "or_not_g"): (122, 119, 106, 100, 119), ("EQ+2", "equiv"): (122, 122, 103, 124, 122),
    ("LT+2", "or_g"): (129, 15, 210, 55, 15), ("LT+2", "or_not_g"): (129, 15, 210, 55, 15), ("LT+2", "equiv"): (129, 129, 96, 146, 129),
    ("LTconst", "or_g"): (9, 6, 9, 6, 6), ("LTconst", "or_not_g"): (9, 6, 9, 6, 6), ("LTconst", "equiv"): (9, 9, 6, 12, 9),
    ("LTsum", "or_g"): (1257, 813, 2562, 738, 813), ("LTsum", "or_not_g"): (1257, 813, 2562, 738, 813), ("LTsum", "equiv"): (1257, 1257, 2118, 1284, 1257),
    ("LT3+1", "or_g"): (1257, 444, 2931, 1157, 444), ("LT3+1", "or_not_g"): (1257, 444, 2931, 1157, 444), ("LT3+1", "equiv"): (1257, 1257, 2118, 2589, 1257),
    ("GT3", "or_g"): (1257, 813, 2562, 1432, 813), ("GT3", "or_not_g"): (1257, 813, 2562, 1432, 813), ("GT3", "equiv"): (1257, 1257, 2118, 2589, 1257),
    ("EQ3-1", "or_g"): (1041, 1023, 2352, 1979, 1023), ("EQ3-1", "or_not_g"): (1041, 1023, 2352, 1979, 1023),
    ("EQ3+0", "or_g"): (907, 888, 2487, 2056, 888), ("EQ3+0", "or_not_g"): (907, 888, 2487, 2056, 888),
    ("EQ3+1", "or_g"): (1041, 1023, 2352, 1979, 1023), ("EQ3+1", "or_not_g"): (1041, 1023, 2352, 1979, 1023),
    ("BOOL-2", "or_g"): (4, 3, 6, 5, 3), ("BOOL-2", "or_not_g"): (4, 3, 6, 5, 3), ("BOOL-2", "equiv"): (4, 4, 4, 8, 4),
    ("NBOOL-2", "or_g"): (4, 1, 8, 5, 1), ("NBOOL-2", "or_not_g"): (4, 1, 8, 5, 1), ("NBOOL-2", "equiv"): (4, 4, 4, 8, 4),
    ("MUL3", "or_g"): (927, 913, 1787, 1199, 913), ("MUL3", "or_not_g"): (927, 913, 1787, 1199, 913),
}
# ... over sets (the same figures in both word layouts: a layout moves bits, not values)
SET_COUNTS = {
    ("NEQ-1", "or_g"): (265, 4, 957, 120, 4), ("NEQ-1", "or_not_g"): (265, 4, 957, 120, 4), ("NEQ-1", "equiv"): (265, 265, 696, 805, 265),
    ("EQ-1", "or_g"): (265, 261, 700, 685, 261), ("EQ-1", "or_not_g"): (265, 261, 700, 685, 261), ("EQ-1", "equiv"): (265, 265, 696, 805, 265),
    ("LT-1", "or_g"): (274, 257, 704, 677, 257), ("LT-1", "or_not_g"): (274, 257, 704, 677, 257), ("LT-1", "equiv"): (274, 274, 687, 913, 274),
    ("NEQ+0", "or_g"): (185, 5, 956, 150, 5), ("NEQ+0", "or_not_g"): (185, 5, 956, 150, 5), ("NEQ+0", "equiv"): (185, 185, 776, 900, 185),
    ("EQ+0", "or_g"): (185, 180, 781, 750, 180), ("EQ+0", "or_not_g"): (185, 180, 781, 750, 180), ("EQ+0", "equiv"): (185, 185, 776, 900, 185),
    ("LT+0", "or_g"): (178, 129, 832, 720, 129), ("LT+0", "or_not_g"): (178, 129, 832, 720, 129), ("LT+0", "equiv"): (178, 178, 783, 1179, 178),
    ("NEQ+2", "or_g"): (372, 3, 958, 90, 3), ("NEQ+2", "or_not_g"): (372, 3, 958, 90, 3), ("NEQ+2", "equiv"): (372, 372, 589, 675, 372),
    ("EQ+2", "or_g"): (372, 369, 592, 585, 369), ("EQ+2", "or_not_g"): (372, 369, 592, 585, 369), ("EQ+2", "equiv"): (372, 372, 589, 675, 372),
    ("LT+2", "or_g"): (274, 17, 944, 236, 17), ("LT+2", "or_not_g"): (274, 17, 944, 236, 17), ("LT+2", "equiv"): (274, 274, 687, 913, 274),
    ("LTconst", "or_g"): (10, 7, 24, 21, 7), ("LTconst", "or_not_g"): (10, 7, 24, 21, 7), ("LTconst", "equiv"): (10, 10, 21, 42, 10),
    ("LT3+1", "or_g"): (1522, 524, 4201, 1663, 524), ("LT3+1", "or_not_g"): (1522, 524, 4201, 1663, 524), ("LT3+1", "equiv"): (1522, 1522, 3203, 3780, 1522),
    ("GT3", "or_g"): (1522, 998, 3727, 2117, 998), ("GT3", "or_not_g"): (1522, 998, 3727, 2117, 998), ("GT3", "equiv"): (1522, 1522, 3203, 3780, 1522),
    ("EQ3-1", "or_g"): (1254, 1236, 3489, 2865, 1261), ("EQ3-1", "or_not_g"): (1254, 1236, 3489, 2865, 1261),
    ("EQ3+0", "or_g"): (1067, 1048, 3677, 2949, 1075), ("EQ3+0", "or_not_g"): (1067, 1048, 3677, 2949, 1075),
    ("EQ3+1", "or_g"): (1254, 1236, 3489, 2867, 1259), ("EQ3+1", "or_not_g"): (1254, 1236, 3489, 2867, 1259),
    ("BOOL-2", "or_g"): (4, 3, 8, 7, 3), ("BOOL-2", "or_not_g"): (4, 3, 8, 7, 3), ("BOOL-2", "equiv"): (4, 4, 4, 8, 4),
    ("NBOOL-2", "or_g"): (4, 1, 10, 7, 1), ("NBOOL-2", "or_not_g"): (4, 1, 10, 7, 1), ("NBOOL-2", "equiv"): (4, 4, 4, 8, 4),
}


def test_the_tables_are_complete():
    assert sorted(INTERVAL_COUNTS) == sorted(LC.INTERVAL_TABLES) and sorted(SET_COUNTS) == sorted(LC.SET_TABLES)
    assert {n for n, _ in LC.INTERVAL_TABLES} - {n for n, _ in LC.SET_TABLES} == {"LTsum", "MUL3"}
    for n in ("EQ3-1", "EQ3+0", "EQ3+1", "MUL3"):
        assert (n, "equiv") not in INTERVAL_COUNTS
        with pytest.raises(M.ContractViolation):
            M.not_(LC.VARIANTS[n][1]([M.Identity(0), M.Identity(1), M.Identity(2)]))
    sizes = {n: len(LC.interval_table(n, "or_g")[2]) for n in LC.VARIANTS}
    assert sizes["EQ+0"] == 225 * 3 and sizes["GT3"] == sizes["EQ3+0"] == sizes["LTsum"] == 3375 * 3 and sizes["LTconst"] == 15 * 3
    assert sizes["MUL3"] == 45 * 10 * 6 * 3 and sizes["BOOL-2"] == (4 + 5) * 3 and len(LC.interval_table("BOOL-2", "equiv")[2]) == (4 + 4) * 3
    assert len(LC.set_table("EQ+0", "or_g", 1, -2)[2]) == 31 * 31 * 3 and len(LC.set_table("GT3", "or_g", 1, -2)[2]) == (3375 + 6 * 225) * 3


@pytest.mark.parametrize("name,form", LC.INTERVAL_TABLES, ids=[f"{n}-{f}" for n, f in LC.INTERVAL_TABLES])
def test_interval_table(name, form):
    got = LC.interval_table_counts(name, form)
    print(name, form, got)
    assert min(got) > 0 and got == INTERVAL_COUNTS[name, form]
    _, _, L, U, open_ = LC.interval_table(name, form)
    assert open_.sum() * 3 == len(open_) and (L[open_, -1] == 0).all() and (U[open_, -1] == 1).all() and (L[~open_, -1] == U[~open_, -1]).all()


@pytest.mark.parametrize("sw,base", LC.SET_LAYOUTS)
@pytest.mark.parametrize("name,form", LC.SET_TABLES, ids=[f"{n}-{f}" for n, f in LC.SET_TABLES])
def test_set_table(name, form, sw, base):
    got = LC.set_table_counts(name, form, sw, base)
    print(name, form, sw, base, got)
    assert min(got) > 0 and got == SET_COUNTS[name, form]
    bits = LC.set_table(name, form, sw, base)[2]
    if sw == 2:  # -1 is bit 63 of word 0, 0 is bit 0 of word 1
        assert (bits[:, :, 1] & np.uint64(1)).any() and ((bits[:, :, 0] >> np.uint64(63)).any() or name.startswith(("BOOL", "NBOOL")))


def test_three_operand_set_tables_have_holes():
    bits = LC.set_table("EQ3+0", "or_g", 1, -2)[2]
    x = bits[:, 0, 0]
    holed = (x & (x >> np.uint64(2)) & ~(x >> np.uint64(1))) != 0  # v and v + 2 without v + 1
    assert holed.sum() == 6 * 225 * 3 and not ((bits[:, 1, 0] & (bits[:, 1, 0] >> np.uint64(2)) & ~(bits[:, 1, 0] >> np.uint64(1))) != 0).any()


# ------------------------------------------------------------------------------------------------------------- random stores
ALL_KINDS = {M.NEQ, M.EQ, M.LT, M.LT3, M.GT3, M.EQ3, M.MUL3, M.BOOL, M.NBOOL}


@pytest.mark.parametrize("name", LC.RANDOM_CASES)
def test_random_case(name):
    """Seeds 7101-7104 (0, 6), 7111-7114 (-4, 5), 7128 and 7122-7124 (-9, -2); the set-mode stores use seed + 50.  At least 10 % of the
    nodes are not failed and narrowed — only those compare rows —, a node ends True, every kind the mode allows is in the lowered leaf
    tables (and a Sum operand in interval mode), and the shapes are the ones the kernels branch on."""
    seed, dom, n_units, n_vars = LC.RANDOM_CASES[name]
    vs, cs, sol, L, U = LC.random_case(name)
    assert len(vs) == n_vars and len(cs) == n_units and L.shape == (LC.N_NODES, n_vars)
    kinds, has_sum = LC.leaf_kinds(cs, len(vs))
    assert kinds == ALL_KINDS and has_sum
    assert all(LC.holds(u, sol) for u in cs.units)
    lb, ub, act, st = LC.random_reference(name)
    narrowed = (st != M.FALSE) & ((lb != L) | (ub != U)).any(axis=1)
    print(name, "interval: narrowed", int(narrowed.sum()), "True", int((st == M.TRUE).sum()), "False", int((st == M.FALSE).sum()))
    assert 10 * narrowed.sum() >= LC.N_NODES and (st == M.TRUE).any() and (st == M.UNKNOWN).any()
    assert (L[:, : n_vars - 6].min(), U[:, : n_vars - 6].max()) == dom

    vs, cs, sol, bits, sw, base = LC.set_random_case(name)
    assert len(vs) == n_vars and len(cs) == n_units and bits.shape == (LC.N_NODES, n_vars, sw)
    kinds, has_sum = LC.leaf_kinds(cs, len(vs))
    assert kinds == ALL_KINDS - {M.MUL3} and not has_sum
    assert all(LC.holds(u, sol) for u in cs.units)
    lb, ub, out, act, st = LC.set_random_reference(name)
    narrowed = (st != M.FALSE) & (out != bits).any(axis=(1, 2))
    print(name, "sets: narrowed", int(narrowed.sum()), "True", int((st == M.TRUE).sum()), "False", int((st == M.FALSE).sum()))
    assert 10 * narrowed.sum() >= LC.N_NODES and (st == M.TRUE).any() and (st == M.UNKNOWN).any()


def test_random_cases_cover_the_shapes():
    """Wu = 1, 2, 3 and 5 `active` words of 32 bits (odd counts: the last 64-bit word is half used), 1, 2 and 3 words of 64; variable
    counts on both sides of 32 and 64; every domain at every unit count; a random row switches units off, the last-unit row all but one."""
    cases = LC.RANDOM_CASES.values()
    assert {(u + 31) // 32 for _, _, u, _ in cases} == {1, 2, 3, 5} and {(u + 63) // 64 for _, _, u, _ in cases} == {1, 2, 3}
    assert {v for _, _, _, v in cases} == {12, 40, 70}
    assert {(d, u) for _, d, u, _ in cases} == {(d, u) for d in ((0, 6), (-4, 5), (-9, -2)) for u in (6, 34, 66, 130)}
    full = LC.active_rows("full", 5, 130, 1)
    assert full.shape == (5, 3) and int(full[0, 2]) == 3
    last = LC.active_rows("last", 5, 130, 1)
    assert last[:, :2].sum() == 0 and (last[:, 2] == 2).all()
    for kind, lo, hi in (("off10", 0.05, 0.15), ("off50", 0.4, 0.6)):
        a = LC.active_rows(kind, LC.N_NODES, 130, 1)
        off = 1 - sum(bin(int(w)).count("1") for w in a.reshape(-1)) / (LC.N_NODES * 130)
        assert lo < off < hi and (a[:, 2] >> np.uint64(2) == 0).all()
    for name in ("p130", "z66"):  # switching units off changes what the oracle answers
        assert any(not np.array_equal(LC.random_reference(name)[3], LC.random_reference(name, k)[3]) for k in ("off50", "last"))


def test_forest_stores():
    """The three interval stores and the three set stores the forests run on: what the oracle's search gives within 2000 nodes.  On the
    domains with values below zero MiddleVal truncates toward zero, the left child of (-1, 0) or (-9, -8) is its parent again, and the
    reference descends without end (test_form_forest_gpu.test_values_at_and_below_zero): 2000 nodes, no leaf."""
    want = {"p34": ((2000, 464, 497), (2000, 954, 0)), "z34": ((2000, 0, 0), (2000, 0, 0)), "n34": ((2000, 0, 0), (2000, 0, 0))}
    for name in LC.FOREST_CASES:
        vs, cs, _, _, _ = LC.random_case(name)
        lb0, ub0 = vs.bounds()
        ss = LC.oracle_model(vs, cs).search(lb0, ub0, all_solutions=True, node_limit=2000)[0]
        vs, cs, _, _, sw, base = LC.set_random_case(name)
        lb0, ub0 = vs.bounds()
        st = LC.oracle_model(vs, cs).search_set(lb0, ub0, sw, base, all_solutions=True, node_limit=2000)[0]
        got = tuple((s["num_nodes"], s["num_solution"], s["num_failed_node"]) for s in (ss, st))
        print(name, got)
        assert got == want[name]


# ------------------------------------------------------------------------------------------------------------- mask edges
def test_mask_edge_nodes_do_what_they_were_built_for():
    vs, cs, L, U = LC.mask_edge_case()
    y0, z0 = 13, 76
    for set_mode in (False, True):
        ref = LC.mask_edge_reference(set_mode)
        lb, ub, act, st = ref[0], ref[1], ref[-2], ref[-1]
        mode = np.arange(LC.N_EDGE) % 4
        assert ((st == M.FALSE) == (mode == 2)).all() and (st != M.TRUE).all()   # every child disentailed: the node fails, and only then
        moved = (lb != L) | (ub != U)
        one, two, ent = mode == 0, mode == 1, mode == 3
        # one child open: it is propagated (y_i < 0 takes 0..3 away) and the unit is entailed; two open: nothing moves, the unit stays
        assert (moved[one, y0:z0].sum(axis=1) == 1).all() and not moved[two, y0:z0].any() and not moved[ent, y0:z0].any()
        unit = lambda u: ((act[:, 0] >> np.uint64(u)) & np.uint64(1)).astype(bool)
        assert not unit(2)[one].any() and unit(2)[two].all() and not unit(2)[ent].any()
        assert moved[0, y0 + 62] and ub[0, y0 + 62] == -1          # bit 63 of the Or of 63: the last leaf, propagated
        assert L[3, y0 + 62] == -2 and U[3, y0 + 62] == -1          # ... and entailed
        assert moved[0, z0 + 60] and lb[0, z0 + 60] == 2            # bit 63 of the And of two Ors
        assert (moved[one | two | ent, z0:].sum(axis=1) >= 1).all()  # the half with one open child is propagated
        assert not unit(3)[one].any() and unit(3)[two].all()
        assert unit(4)[st != M.FALSE].all() and moved[st != M.FALSE, :12].any(axis=1).all()  # the Distinct of 67 nodes narrows and stays
    nodes, leaves = M.lower_formula(LC.not_flat_65()[1].units[1], 63)
    assert len(nodes) == 65 and nodes[0]["type"] == M.F_AND and nodes[1]["type"] == M.F_OR and nodes[1]["n_children"] == 63
