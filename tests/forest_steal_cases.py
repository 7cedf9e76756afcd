"""What pcp_dfs_forest_steal must do, restated in numpy from its contract in include/pcp_hip.h (not by calling run_forest_loop), and random
forest states to run it on.  Shared by test_forest_steal_cpu.py and test_forest_steal_gpu.py.

A state is a dict of numpy arrays: ``lb`` / ``ub`` [T, capacity, V] int32, ``sp`` [T] int32, ``dirty`` [T, capacity] int32 or None, and — the
exclusion state, all three None without it — ``row_base`` [T, capacity] int32, ``row_excl`` [T, capacity, 2] int32, ``path``
[T, max(path_capacity, 1), 2] int32, with ``path_capacity`` (what the entry is told) and ``capacity``."""
import numpy as np

ARRAYS = ("lb", "ub", "sp", "dirty", "row_base", "row_excl", "path")
ROW_ARRAYS = ("lb", "ub", "dirty", "row_base", "row_excl")
STALE = -0x5A5A5A  # rows at or above sp hold this (minus the tree's index): recognisable in a row that should not have moved


def copy_state(s):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}


def pair_valid(s, d, r):
    """The contract's verdict on one pair, on the state ``s`` as it is."""
    T = len(s["sp"])
    d, r = int(d), int(r)
    if d == r or not (0 <= d < T) or not (0 <= r < T):
        return False
    if int(s["sp"][r]) != 0 or not (2 <= int(s["sp"][d]) <= s["capacity"]):
        return False
    if s["row_base"] is not None and int(s["row_base"][d, 0]) > s["path_capacity"]:
        return False
    return True


def steal_reference(state, pairs):
    """(state', done): every pair judged on ``state`` as it came, the valid ones then carried out one after the other (a tree is in at most
    one valid pair, so their order does not matter).  ``pairs``: [n, 2] integers, read as uint32."""
    pairs = np.asarray(pairs).reshape(-1, 2).astype(np.int64) & 0xFFFFFFFF
    done = np.array([1 if pair_valid(state, d, r) else 0 for d, r in pairs], np.int32)
    s = copy_state(state)
    for (d, r), ok in zip(pairs, done):
        if not ok:
            continue
        k = int(s["sp"][d])
        if s["row_base"] is not None:
            nb = int(s["row_base"][d, 0])
            s["path"][r, :nb] = s["path"][d, :nb]
            s["row_base"][r, 0] = nb
            s["row_excl"][r, 0] = s["row_excl"][d, 0]
        for name in ROW_ARRAYS:
            a = s[name]
            if a is None:
                continue
            if name in ("lb", "ub", "dirty"):
                a[r, 0] = a[d, 0]
            a[d, 0:k - 1] = a[d, 1:k].copy()
        s["sp"][d] = k - 1
        s["sp"][r] = 1
    return s, done


def random_state(rng, T, capacity, V, sp=None, dirty=True, excl=True, path_capacity=6):
    """A forest state with ``sp`` (given, or random with idle, single-row, deep and full trees mixed).  Rows at or above sp hold STALE - t;
    row_base does not decrease along a tree's rows and stays within path_capacity; about half the rows have an entry of their own."""
    sp = np.asarray(sp, np.int32).copy() if sp is not None else rng.choice([0, 0, 1, 2, capacity, int(rng.integers(0, capacity + 1))], size=T).astype(np.int32)
    s = {"capacity": int(capacity), "path_capacity": int(path_capacity), "sp": sp}
    s["lb"] = rng.integers(-1000, 1000, size=(T, capacity, V)).astype(np.int32)
    s["ub"] = (s["lb"] + rng.integers(0, 50, size=(T, capacity, V))).astype(np.int32)
    s["dirty"] = rng.integers(0, V + 2, size=(T, capacity)).astype(np.int32) if dirty else None
    s["row_base"] = s["row_excl"] = s["path"] = None
    if excl:
        s["row_base"] = np.sort(rng.integers(0, path_capacity + 1, size=(T, capacity)), axis=1).astype(np.int32)
        s["row_excl"] = np.stack([np.where(rng.random((T, capacity)) < 0.5, -1, rng.integers(0, V, size=(T, capacity))),
                                  rng.integers(-1000, 1000, size=(T, capacity))], axis=2).astype(np.int32)
        s["path"] = np.stack([rng.integers(0, V, size=(T, max(path_capacity, 1))), rng.integers(-1000, 1000, size=(T, max(path_capacity, 1)))], axis=2).astype(np.int32)
    for t in range(T):
        for name in ROW_ARRAYS:
            if s[name] is not None:
                s[name][t, min(max(int(sp[t]), 0), capacity):] = STALE - t
    return s


def touched_trees(state, pairs, done):
    pairs = np.asarray(pairs).reshape(-1, 2).astype(np.int64) & 0xFFFFFFFF
    return {int(t) for (d, r), ok in zip(pairs, done) if ok for t in (d, r)}


def assert_steal_matches(before, want, got, pairs, done_want, done_got, what=""):
    """``got`` against the reference's ``want``: done; sp; rows [0, sp) of every row array; path entries [0, row_base[t][0]) of every tree with
    rows; a donor's whole path (it stays as it is); and every tree in no valid pair bit for bit against ``before``."""
    assert np.array_equal(np.asarray(done_got, np.int64), np.asarray(done_want, np.int64)), (what, "done", done_got, done_want)
    assert np.array_equal(got["sp"], want["sp"]), (what, "sp", got["sp"], want["sp"])
    touched = touched_trees(before, pairs, done_want)
    donors = {int(d) & 0xFFFFFFFF for (d, r), ok in zip(np.asarray(pairs).reshape(-1, 2), done_want) if ok}
    for t in range(len(want["sp"])):
        if t not in touched:
            for name in ARRAYS:
                if before[name] is not None:
                    assert np.array_equal(got[name][t], before[name][t]), (what, "untouched tree changed", t, name)
            continue
        n = int(want["sp"][t])
        for name in ROW_ARRAYS:
            if want[name] is not None:
                assert np.array_equal(got[name][t, :n], want[name][t, :n]), (what, "rows", t, name)
        if want["row_base"] is not None:
            nb = int(want["row_base"][t, 0])
            assert np.array_equal(got["path"][t, :nb], want["path"][t, :nb]), (what, "path prefix", t)
            if t in donors:
                assert np.array_equal(got["path"][t], before["path"][t]), (what, "donor's path changed", t)


def host_policy(sp):
    """run_forest_loop's two lists, restated: (donors, idle) — the trees with two or more rows, richest first and ties by index, cut to the
    number of idle trees; the idle trees by index."""
    sp = np.asarray(sp)
    idle = [int(i) for i in np.nonzero(sp == 0)[0]]
    donors = [int(i) for i in np.argsort(-sp.astype(np.int64), kind="stable") if sp[i] >= 2][:len(idle)]
    return donors, idle
