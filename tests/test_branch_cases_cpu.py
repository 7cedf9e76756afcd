"""The cases of branch_cases.py, checked without a GPU: every case has the property it claims — recomputed here from its arrays: where the
Unknown nodes sit relative to the seams of the scan, where the ties are and which thread of a 256-thread block reads them, the word counts —
and the host brancher (pcp_amd.search) equals the scalar reference on every case and on the reference's own selector tables.  Conditions on
the inputs, fixed before any GPU run; no kernel is measured here."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as orc
from pcp_amd import search as S

import branch_cases as B

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def sizes(case):
    return case["ub"].astype(np.int64) - case["lb"].astype(np.int64) + 1


def test_number_of_cases_per_family():
    """No case skipped or filtered out: a generator that silently produces fewer fails here."""
    cases = B.all_cases()
    assert [c["name"] for c in cases] == B.CASE_NAMES and len(set(B.CASE_NAMES)) == len(cases) == 59
    per_family = {f: sum(c["family"] == f for c in cases) for f in B.FAMILY_SIZES}
    assert per_family == B.FAMILY_SIZES == {"scan": 40, "select": 10, "middle": 3, "active": 5, "nosplit": 1}
    assert cases[-1]["family"] == "nosplit"
    assert B.SCAN_SIZES == (1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3100)
    assert B.SELECT_VS == (1, 2, 63, 64, 65, 255, 256, 257, 513, 1000)
    assert B.ACTIVE_UNITS == (1, 64, 65, 320, 16450)
    for c in cases:
        n, V = c["lb"].shape
        assert c["ub"].shape == (n, V) and c["status"].shape == (n,) and c["lb"].dtype == c["ub"].dtype == np.int32
        assert (c["lb"] <= c["ub"]).all() and np.abs(c["lb"].astype(np.int64)).max() <= B.BOUND_MAX and np.abs(c["ub"].astype(np.int64)).max() <= B.BOUND_MAX
        assert (c["active"] is None) == (c["n_units"] == 0)
        # the largest shapes: 3100 nodes x 5 variables, 130 nodes x 258 words, 1000 variables x a few dozen rows
        assert n * V <= 3100 * 5 or (V == 1000 and n <= 36)


@pytest.mark.parametrize("pattern", B.SCAN_PATTERNS)
@pytest.mark.parametrize("n", B.SCAN_SIZES)
def test_scan_cases_put_their_nodes_on_the_seams(n, pattern):
    c = B.case_by_name(f"scan-{n}-{pattern}")
    assert c["lb"].shape == (n, B.SCAN_V) and c["claims"] == {"n_nodes": n, "pattern": pattern}
    st = c["status"]
    unk = st == B.UNKNOWN
    assert (sizes(c)[unk] > 1).any(axis=1).all()  # every Unknown row can be split
    assert B.fits_cells(c).all()
    # the seams, recomputed: the first and the last index of every span of 64 (a wavefront) and of 1024 (a chunk of the loop) that exists
    edge = set()
    for span in (64, B.SCAN_BLOCK):
        for first in range(0, n, span):
            edge |= {first, min(first + span - 1, n - 1)}
    assert edge == set(B.seams(n).tolist())
    edge = np.array(sorted(edge))
    if pattern == "all_unknown":
        assert unk.all()
    elif pattern == "no_unknown":
        assert not unk.any() and (n < 63 or set(st.tolist()) == {0, 1, B.HULL})
    else:
        assert unk[edge].all() if pattern == "unknown_on_seams" else not unk[edge].any()
        if n >= 63:
            assert set(st.tolist()) == {0, 1, B.UNKNOWN, B.HULL}
            inner = np.setdiff1d(np.arange(n), edge)
            assert unk[inner].any() and (~unk[inner]).any()
    if n > B.SCAN_BLOCK and pattern != "no_unknown":
        # the carry matters: Unknown nodes in the first chunk and in every later one (but a last chunk that is all seam, kept clear of them)
        for first in range(0, n, B.SCAN_BLOCK):
            chunk = np.arange(first, min(first + B.SCAN_BLOCK, n))
            assert unk[chunk].any() or (pattern == "others_on_seams" and np.isin(chunk, edge).all()), first


def _thread(i):
    return i % B.BLOCK, (i % B.BLOCK) // 64, i // B.BLOCK  # thread, its wavefront, the iteration of the strided loop


def test_the_named_tie_pairs_cross_threads_wavefronts_and_iterations():
    """In each pair the lower index is not simply the lower thread of one wavefront in one iteration."""
    t = {p: (_thread(p[0]), _thread(p[1])) for p in B.TIE_PAIRS}
    (ti, wi, ki), (tj, wj, kj) = t[(70, 300)]
    assert ti > tj and wi > wj and ki < kj          # the lower index in a higher thread and wavefront, the higher one an iteration later
    (ti, wi, ki), (tj, wj, kj) = t[(1, 256)]
    assert ti > tj and wi == wj and ki < kj         # the lower index in a higher thread of the same wavefront
    (ti, wi, ki), (tj, wj, kj) = t[(63, 64)]
    assert wi + 1 == wj and ki == kj                # neighbours in two wavefronts: the tie is decided in shared memory
    (ti, wi, ki), (tj, wj, kj) = t[(255, 511)]
    assert ti == tj and ki + 1 == kj                # one thread, two iterations: the tie is decided in its register
    present = {tuple(r[1:]) for V in B.SELECT_VS for r in B.case_by_name(f"select-{V}")["claims"]["rows"] if r[0] == "tie"}
    assert present >= set(B.TIE_PAIRS)


@pytest.mark.parametrize("V", B.SELECT_VS)
def test_select_cases_hold_what_they_claim(V):
    c = B.case_by_name(f"select-{V}")
    rows = c["claims"]["rows"]
    size = sizes(c)
    assert c["lb"].shape == (len(rows), V) and (c["status"] == B.UNKNOWN).all() and c["claims"]["V"] == V
    kinds = [r[0] for r in rows]
    want_unique = sorted({i for i in B.UNIQUE_AT if i < V} | {V - 1})
    assert [r[1] for r in rows if r[0] == "unique"] == want_unique
    want_ties = sorted({p for p in B.TIE_PAIRS if p[1] < V} | ({(0, V - 1)} if V >= 2 else set()))
    assert [tuple(r[1:]) for r in rows if r[0] == "tie"] == want_ties
    assert kinds.count("one_free") == 1 and kinds.count("big") == 1 and kinds.count("assigned_first") == (1 if V >= 2 else 0)
    for r, claim in enumerate(rows):
        s = size[r]
        cand = np.nonzero(s > 1)[0]
        least = s[cand].min()
        at_min = cand[s[cand] == least].tolist()
        if claim[0] == "unique":
            assert at_min == [claim[1]] and (V == 1 or len(cand) == V)
        elif claim[0] == "one_free":
            assert cand.tolist() == [claim[1]]
        elif claim[0] == "tie":
            assert at_min == [claim[1], claim[2]] and claim[1] < claim[2] and len(cand) == V
        elif claim[0] == "assigned_first":
            assert at_min == [claim[1]] and s[0] == 1 and claim[1] == V - 1 and (s[:claim[1]] == 1).sum() >= 1
        else:
            i, j = claim[1], claim[2]
            if j is None:
                assert V == 1 and cand.tolist() == [0] and s[0] == B.BIG_SIZES[1]
            else:
                assert cand.tolist() == [i, j] and i < j and (s[i], s[j]) == (B.BIG_SIZES[1], B.BIG_SIZES[0])
                assert (c["lb"][r, i], c["ub"][r, i]) == (-B.BOUND_MAX, B.BOUND_MAX)
            assert not B.fits_cells(c)[r]
    assert B.fits_cells(c).sum() == len(rows) - 1  # every other row can go through the cell format


@pytest.mark.parametrize("which", list(B.MIDDLE_WINDOWS))
def test_middle_cases_cover_their_windows_and_the_negative_odd_sums(which):
    c = B.case_by_name(f"middle-{which}")
    doms = c["claims"]["doms"]
    n_window = sum((hi - lo + 1) * (hi - lo) // 2 for lo, hi in B.MIDDLE_WINDOWS[which])
    assert len(doms) == n_window + len(B.MIDDLE_SPANS[which]) == {"small": 78, "cell_edge": 45, "row_edge": 45}[which]
    assert c["lb"].shape == (len(doms), 3) and (sizes(c) > 1).sum(axis=1).tolist() == [1] * len(doms)
    limit = {"small": 6, "cell_edge": B.CELL_MAX, "row_edge": B.BOUND_MAX}[which]
    assert int(c["lb"].min()) == -limit and int(c["ub"].max()) == limit
    assert B.fits_cells(c).all() == (which != "row_edge")
    stuck = 0
    for r, (a, b) in enumerate(doms):
        var, (l0, u0), (l1, u1) = B.ref_children(c["lb"][r], c["ub"][r])
        assert var == r % 3 and (c["lb"][r, var], c["ub"][r, var]) == (a, b)
        v = u0[var]
        assert 2 * v in (a + b - 1, a + b, a + b + 1) and l1[var] == v + 1 and (l0[var], u1[var]) == (a, b)
        if (a + b) % 2 and a + b < 0:
            assert 2 * v == a + b + 1  # toward zero: not the floor
            if b == a + 1:
                # the reference's left child is its parent again, the right one empty
                assert (l0, u0) == (c["lb"][r].tolist(), c["ub"][r].tolist()) and l1[var] == u1[var] + 1
                stuck += 1
        else:
            assert a <= v < b
    assert stuck >= 3
    assert sum((a + b) % 2 == 1 and a + b < 0 and b > a + 1 for a, b in doms) >= 3


@pytest.mark.parametrize("n_units,words", list(zip(B.ACTIVE_UNITS, B.ACTIVE_WORDS)))
def test_active_cases_fill_their_words_and_keep_the_tail_clear(n_units, words):
    c = B.case_by_name(f"active-{n_units}")
    act = c["active"]
    assert c["lb"].shape == (B.ACTIVE_NODES, B.ACTIVE_V) == (130, 9) and act.shape == (130, words) and act.dtype == np.uint64
    assert (n_units + 63) // 64 == words == c["claims"]["words"] and (words > B.BLOCK) == (n_units == 16450)
    tail = n_units % 64
    if tail:
        assert not (act[:, -1] >> np.uint64(tail)).any()
    assert (act != 0).any(axis=0).all() and len(np.unique(act[:, -1])) > 1  # no column, the last one included, is constant
    assert set(c["status"].tolist()) == {0, 1, B.UNKNOWN, B.HULL}
    props = B.units_model(B.ACTIVE_V, n_units)
    assert len({(int(p["var"][0]), int(p["var"][1]), int(p["off"][1])) for p in props}) == n_units
    assert orc.OracleModel(B.ACTIVE_V, props).n_units == n_units


def test_the_row_with_nothing_to_split_sits_in_the_middle():
    c = B.all_cases()[-1]
    r = c["claims"]["row"]
    assert (c["status"] == B.UNKNOWN).all() and 0 < r < len(c["lb"]) - 1
    assert (sizes(c)[r] == 1).all() and (np.delete(sizes(c), r, axis=0) > 1).any(axis=1).all()
    e = B.expected(c["lb"], c["ub"], c["status"])
    assert e["dirty"][2 * r] == e["dirty"][2 * r + 1] == B.NOVAR and (np.delete(e["dirty"], [2 * r, 2 * r + 1]) < c["lb"].shape[1]).all()
    for k in (2 * r, 2 * r + 1):
        assert np.array_equal(e["child_lb"][k], c["lb"][r]) and np.array_equal(e["child_ub"][k], c["ub"][r])
    with pytest.raises(RuntimeError):
        S.branch(c["lb"][r:r + 1], c["ub"][r:r + 1], None)
    with pytest.raises(orc.OraclePanic):
        orc.first_smallest_var(list(zip(c["lb"][r].tolist(), c["ub"][r].tolist())))


@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_host_brancher_equals_the_scalar_reference(name):
    """pcp_amd.search.first_smallest_var / middle_val / branch against the plain-integer restatement: two statements of the brancher that
    share no code, so the device is held to both."""
    c = B.case_by_name(name)
    lb, ub, status, active = c["lb"], c["ub"], c["status"], c["active"]
    want_var = [B.ref_var(lb[i], ub[i]) for i in range(len(lb))]
    got_var = S.first_smallest_var(lb, ub)
    assert got_var.tolist() == [-1 if v is None else v for v in want_var]
    has = np.array([v is not None for v in want_var])
    rows = np.nonzero(has)[0]
    var = got_var[rows]
    assert S.middle_val(lb[rows, var], ub[rows, var]).tolist() == [B.ref_middle(lb[r, v], ub[r, v]) for r, v in zip(rows, var)]
    keep = has & (status == B.UNKNOWN)
    e = B.expected(lb[keep], ub[keep], status[keep], None if active is None else active[keep])
    assert e["counts"] == [2 * int(keep.sum()), 0, 0, int(keep.sum()), 0]
    L, U, A = S.branch(lb[keep], ub[keep], None if active is None else active[keep])
    assert np.array_equal(L, e["child_lb"]) and np.array_equal(U, e["child_ub"])
    assert (A is None and e["child_active"] is None) or np.array_equal(A, e["child_active"])
    assert e["dirty"].tolist() == np.repeat(var[keep[rows]], 2).tolist()
    # the whole batch: the counts are the statuses', the children those of the Unknown rows in order
    full = B.expected_by_name(name)
    n_unk = int((status == B.UNKNOWN).sum())
    assert full["counts"] == [2 * n_unk, int((status == 1).sum()), int((status == 0).sum()), n_unk, int((status > B.UNKNOWN).sum())]
    assert full["child_lb"].shape == (2 * n_unk, lb.shape[1]) and full["counts"][4] == int((status == B.HULL).sum())


def test_reference_and_host_brancher_on_the_reference_tables():
    """first_smallest_var.rs:63-72 and binary_split.rs:108-133, as transcribed into tests/golden/engine_kats.json."""
    g = json.load(open(os.path.join(GOLDEN, "engine_kats.json")))["search"]
    for case in g["first_smallest_var"]["cases"]:
        lb = np.array([[d[0] for d in case["vars"]]], np.int32); ub = np.array([[d[1] for d in case["vars"]]], np.int32)
        assert B.ref_var(lb[0], ub[0]) == case["expect"] == int(S.first_smallest_var(lb, ub)[0])
    panic = g["first_smallest_var"]["panic"]["vars"]
    lb = np.array([[d[0] for d in panic]], np.int32); ub = np.array([[d[1] for d in panic]], np.int32)
    assert B.ref_var(lb[0], ub[0]) is None and int(S.first_smallest_var(lb, ub)[0]) == -1
    with pytest.raises(RuntimeError):
        S.branch(lb, ub, None)
    root = g["binary_split"]["root"]
    for case in g["binary_split"]["cases"]:  # make var k the smallest non-assigned one
        k = case["var"]
        doms = [[5, 5]] * 3
        doms[k] = root[k]
        lb = np.array([[d[0] for d in doms]], np.int32); ub = np.array([[d[1] for d in doms]], np.int32)
        var, (l0, u0), (l1, u1) = B.ref_children(lb[0], ub[0])
        assert var == k and [[l0[k], u0[k]], [l1[k], u1[k]]] == case["children"]
        assert B.ref_middle(*root[k]) == int(S.middle_val(lb[:, k], ub[:, k])[0]) == case["children"][0][1]
        L, U, _ = S.branch(lb, ub, None)
        assert [[int(L[0, k]), int(U[0, k])], [int(L[1, k]), int(U[1, k])]] == case["children"]
