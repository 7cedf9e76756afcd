"""The host side of Enumerate (search/branching/enumerate.rs:33-60): search.branch_enumerate, the brancher whose right children carry value
exclusions for pcp_propagate_device_excl.  The reference's own distribution vectors (tests/golden/enumerate_kats.json), the interior case the
reference has no vector for, inheritance, and the ABI list."""
import json
import os

import numpy as np
import pytest

import pcp_amd.engine as E
from pcp_amd import search as S


def _rows(root):
    r = np.asarray(root, np.int32)
    return r[None, :, 0].copy(), r[None, :, 1].copy()


def test_reference_distribution_vectors(golden_dir):
    kats = json.load(open(os.path.join(golden_dir, "enumerate_kats.json")))
    assert len(kats["distribution"]) == 3
    for k in kats["distribution"]:
        lb, ub = _rows(k["root"])
        L, U, off, excl, dirty = S.branch_enumerate(lb, ub, None, None, val=k["val"], var=k["var"])
        x = k["var"]
        # MinVal picks a bound, so x != v folds into the bound: no exclusion is left, and the children's bounds are the reference's domains
        assert [[int(L[c, x]), int(U[c, x])] for c in (0, 1)] == k["children"], k["source"]
        assert off.tolist() == [0, 0, 0] and excl.shape == (0, 2), k["source"]
        assert dirty.tolist() == [x, x]
        others = [i for i in range(lb.shape[1]) if i != x]
        for c in (0, 1):
            assert np.array_equal(L[c, others], lb[0, others]) and np.array_equal(U[c, others], ub[0, others])
    for k in kats["impossible"]:
        lb, ub = _rows(k["root"])
        with pytest.raises(RuntimeError):
            S.branch_enumerate(lb, ub, None, None, val=k["val"], var=k["var"])
    # without a given variable FirstSmallestVar picks it: (1, 2) of the reference's root, and an all-assigned space raises as well
    lb, ub = _rows(kats["distribution"][0]["root"])
    assert S.branch_enumerate(lb, ub, None, None, val="min")[4].tolist() == [2, 2]
    with pytest.raises(RuntimeError):
        S.branch_enumerate(*_rows([[1, 1]]), None, None, val="min")


def test_interior_middle_value_becomes_an_exclusion():
    lb, ub = _rows([[1, 10]])
    L, U, off, excl, dirty = S.branch_enumerate(lb, ub, None, None, val="middle")
    assert (int(L[0, 0]), int(U[0, 0])) == (5, 5)    # x = 5 first (enumerate.rs:48-53)
    assert (int(L[1, 0]), int(U[1, 0])) == (1, 10)   # x != 5 removes nothing from an interval (x_neq_y.rs:82-93)
    assert off.tolist() == [0, 0, 1] and excl.tolist() == [[0, 5]]
    assert excl.dtype == np.int32 and off.dtype == np.int32 and excl.flags["C_CONTIGUOUS"]


def test_children_inherit_only_exclusions_still_inside_their_domain():
    # parent: x0 in [1, 10] with 5 and 7 excluded, x1 in [1, 4] with 3 excluded; FirstSmallestVar picks x1, MiddleVal 2 (interior)
    lb, ub = _rows([[1, 10], [1, 4]])
    excl = np.array([[0, 5], [0, 7], [1, 3]], np.int32)
    L, U, off, ex2, dirty = S.branch_enumerate(lb, ub, np.array([0, 3]), excl, val="middle")
    assert dirty.tolist() == [1, 1]
    left, right = ex2[off[0]:off[1]].tolist(), ex2[off[1]:off[2]].tolist()
    assert (int(L[0, 1]), int(U[0, 1])) == (2, 2)
    assert left == [[0, 5], [0, 7]]                     # (1, 3) lies outside x1 = 2: dropped
    assert right == [[0, 5], [0, 7], [1, 3], [1, 2]]    # inherited in order, the new one behind them (Store::alloc order)
    # a fold can land a bound ON an inherited exclusion: it stays with the child (its value is inside the domain) and the engine removes it
    L, U, off, ex2, _ = S.branch_enumerate(lb, ub, np.array([0, 1]), np.array([[1, 2]], np.int32), val="min")
    assert (int(L[1, 1]), int(U[1, 1])) == (2, 4) and ex2[off[0]:off[1]].tolist() == [] and ex2[off[1]:off[2]].tolist() == [[1, 2]]
    # two parents in one call, the second without exclusions; MinVal folds, and the folded bound drops what fell outside
    lb2, ub2 = np.array([[1, 3], [1, 5]], np.int32), np.array([[10, 6], [10, 6]], np.int32)
    L, U, off, ex2, dirty = S.branch_enumerate(lb2, ub2, np.array([0, 2, 2]), np.array([[1, 4], [1, 5]], np.int32), val="min")
    assert dirty.tolist() == [1, 1, 1, 1]
    assert (int(L[1, 1]), int(U[1, 1])) == (4, 6) and (int(L[3, 1]), int(U[3, 1])) == (6, 6)
    assert [ex2[off[i]:off[i + 1]].tolist() for i in range(4)] == [[], [[1, 4], [1, 5]], [], []]


def test_abi_list_names_the_entry():
    assert "pcp_propagate_device_excl" in E.ABI_SYMBOLS  # (tests/test_abi.py then checks the header declares it and the library exports it)


def test_an_excluded_value_is_not_chosen_again():
    """An interior x != v leaves the interval as it is: the right child is its parent again and MiddleVal would pick v for ever.  The brancher
    takes the nearest value the node has not excluded yet, the lower one first."""
    lb, ub = _rows([[1, 10]])
    for have, want in (([5], 4), ([5, 4], 6), ([5, 4, 6], 3)):
        ex = np.array([[0, w] for w in have], np.int32)
        L, U, off, ex2, _ = S.branch_enumerate(lb, ub, np.array([0, len(have)]), ex, val="middle")
        assert (int(L[0, 0]), int(U[0, 0])) == (want, want)
        assert ex2[off[1]:off[2]].tolist() == [[0, w] for w in have] + [[0, want]]
    with pytest.raises(RuntimeError):
        S.branch_enumerate(*_rows([[1, 2]]), np.array([0, 2]), np.array([[0, 1], [0, 2]], np.int32), val="middle")
