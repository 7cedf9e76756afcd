"""The steal between Interval forest trees, without a GPU: search_forest.plan_steal_pairs forms the pairs run_forest_loop's host steal forms,
and tests/forest_steal_cases.steal_reference — the contract of pcp_dfs_forest_steal restated — is what that host steal does today."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from pcp_amd.search_forest import ForestStacks, plan_steal_pairs, run_forest_loop  # noqa: E402
import forest_steal_cases as FC  # noqa: E402


def check_plan(sp, n_pairs, capacity=1 << 20):
    sp = np.asarray(sp, np.int32)
    T = len(sp)
    pairs = plan_steal_pairs(torch.from_numpy(sp.copy()), n_pairs)
    assert pairs.dtype == torch.int32 and tuple(pairs.shape) == (n_pairs, 2)
    pairs = pairs.numpy()
    assert ((pairs >= 0) & (pairs < T)).all()
    donors, idle = FC.host_policy(sp)
    host = list(zip(donors, idle))
    state = {"sp": sp, "capacity": capacity, "row_base": None, "path_capacity": 0}
    valid = [i for i in range(n_pairs) if FC.pair_valid(state, *pairs[i])]
    # the valid pairs are a prefix, pair i is the host's i-th, and together they are the host's zip (cut to n_pairs)
    assert valid == list(range(len(valid))), (sp, pairs)
    for i in valid:
        assert (int(pairs[i, 0]), int(pairs[i, 1])) == host[i], (i, sp, pairs)
    assert len(valid) == min(len(host), n_pairs), (sp, pairs, host)
    # no tree twice among the valid pairs
    used = [int(t) for i in valid for t in pairs[i]]
    assert len(used) == len(set(used))
    return pairs


SHAPES = {
    "one_tree_live": [3],
    "one_tree_idle": [0],
    "all_idle": [0, 0, 0, 0, 0],
    "no_donor_all_one": [1, 1, 1, 1],
    "no_donor_ones_and_idle": [1, 0, 1, 0, 0, 1],
    "more_idle_than_donors": [0, 5, 0, 0, 2, 0, 1, 0],
    "more_donors_than_idle": [4, 5, 0, 3, 2, 9, 1, 7],
    "ties": [3, 0, 3, 2, 0, 3, 2, 0, 2, 0, 3],
    "no_idle": [2, 3, 4, 1],
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_planner_forms_the_host_pairs(name):
    sp = SHAPES[name]
    for n in sorted({0, sum(1 for x in sp if x == 0), len(sp)}):
        check_plan(sp, n)


def test_planner_on_random_stacks():
    rng = np.random.default_rng(20240521)
    for _ in range(200):
        T = int(rng.integers(2, 301))
        top = int(rng.choice([1, 2, 3, 50]))
        sp = rng.integers(0, top + 1, size=T)
        if rng.random() < 0.5:
            sp[rng.random(T) < 0.5] = 0
        idle = int((sp == 0).sum())
        for n in sorted({0, idle, T, int(rng.integers(0, T + 1))}):
            check_plan(sp, n)


def test_planner_refuses_more_pairs_than_trees():
    with pytest.raises(ValueError):
        plan_steal_pairs(torch.zeros(4, dtype=torch.int32), 5)
    with pytest.raises(ValueError):
        plan_steal_pairs(torch.zeros(4, dtype=torch.int32), -1)


def host_steal_once(state):
    """One turn of run_forest_loop's host steal over CPU tensors: the launch does nothing."""
    t = lambda a: None if a is None else torch.from_numpy(a.copy())
    T = len(state["sp"])
    excl = state["row_base"] is not None
    fs = ForestStacks(t(state["lb"]), t(state["ub"]), None, t(state["sp"]), torch.zeros(T, dtype=torch.int32), torch.zeros((T, 5), dtype=torch.int64),
                      dirty=t(state["dirty"]),
                      **(dict(path=t(state["path"]), row_base=t(state["row_base"]), row_excl=t(state["row_excl"]), path_capacity=state["path_capacity"]) if excl else {}))
    loop = run_forest_loop(lambda: None, fs, max_launches=1)
    got = FC.copy_state(state)
    for name in FC.ARRAYS:
        if state[name] is not None:
            got[name] = getattr(fs, name).numpy()
    return got, loop


@pytest.mark.parametrize("excl", [False, True], ids=["no_path", "path"])
@pytest.mark.parametrize("dirty", [False, True], ids=["no_dirty", "dirty"])
def test_reference_is_todays_host_steal(excl, dirty):
    rng = np.random.default_rng(7 + 2 * excl + dirty)
    for case in range(12):
        T, cap, V = int(rng.integers(2, 40)), int(rng.integers(2, 9)), int(rng.integers(1, 12))
        state = FC.random_state(rng, T, cap, V, dirty=dirty, excl=excl, path_capacity=int(rng.integers(0, 7)))
        pairs = plan_steal_pairs(torch.from_numpy(state["sp"].copy()), T).numpy()
        want, done = FC.steal_reference(state, pairs)
        got, loop = host_steal_once(state)
        assert loop["steals"] == int(done.sum()), case
        FC.assert_steal_matches(state, want, got, pairs, done, done, what=("host loop", case))
        if excl and loop["steals"]:
            d, r = (int(x) for x in pairs[0])
            fsr = loop["first_steal"]
            assert (fsr["donor"], fsr["receiver"]) == (d, r)
            # (on CPU tensors the loop's "before" rows are views of the stack, which the shift then moves: only its list is compared)
            assert np.array_equal(fsr["after"][0], state["lb"][d, 0]) and np.array_equal(fsr["after"][1], state["ub"][d, 0])
            assert np.array_equal(fsr["before"][2], fsr["after"][2])


def test_loop_refuses_bad_steal_settings():
    fs = ForestStacks(torch.zeros((2, 2, 1), dtype=torch.int32), torch.zeros((2, 2, 1), dtype=torch.int32), None, torch.ones(2, dtype=torch.int32),
                      torch.zeros(2, dtype=torch.int32), torch.zeros((2, 5), dtype=torch.int64))

    class TwoRanks:
        @staticmethod
        def get_world_size():
            return 2

        @staticmethod
        def get_rank():
            return 0

    with pytest.raises(ValueError):
        run_forest_loop(lambda: None, fs, max_launches=1, steal="bogus")
    with pytest.raises(ValueError):
        run_forest_loop(lambda: None, fs, max_launches=1, steal="device", stealer=lambda p, d: None, dist=TwoRanks)
    with pytest.raises(ValueError):
        run_forest_loop(lambda: None, fs, max_launches=1, steal="device")


def test_device_loop_on_cpu_tensors_with_a_reference_stealer():
    """steal="device" drives the planner and a stealer; with the numpy reference as the stealer it leaves what the host steal leaves,
    and reports the same steals and first_steal."""
    rng = np.random.default_rng(99)
    for case in range(8):
        T, cap, V = int(rng.integers(2, 30)), int(rng.integers(2, 7)), int(rng.integers(1, 9))
        state = FC.random_state(rng, T, cap, V, dirty=True, excl=True, path_capacity=int(rng.integers(1, 6)))
        host, hloop = host_steal_once(state)
        t = lambda a: torch.from_numpy(a.copy())
        fs = ForestStacks(t(state["lb"]), t(state["ub"]), None, t(state["sp"]), torch.zeros(T, dtype=torch.int32), torch.zeros((T, 5), dtype=torch.int64),
                          dirty=t(state["dirty"]), path=t(state["path"]), row_base=t(state["row_base"]), row_excl=t(state["row_excl"]), path_capacity=state["path_capacity"])

        def stealer(pairs, done):
            now = FC.copy_state(state)
            for name in FC.ARRAYS:
                now[name] = getattr(fs, name).numpy().copy()
            after, ok = FC.steal_reference(now, pairs.numpy())
            for name in FC.ARRAYS:
                getattr(fs, name).copy_(torch.from_numpy(after[name]))
            done.copy_(torch.from_numpy(ok))

        dloop = run_forest_loop(lambda: None, fs, max_launches=1, steal="device", stealer=stealer)
        assert dloop["steals"] == hloop["steals"], case
        n_live = np.asarray(host["sp"])
        for name in FC.ROW_ARRAYS:
            for tr in range(T):
                assert np.array_equal(getattr(fs, name).numpy()[tr, :n_live[tr]], host[name][tr, :n_live[tr]]), (case, name, tr)
        assert np.array_equal(fs.sp.numpy(), host["sp"])
        a, b = dloop["first_steal"], hloop["first_steal"]
        assert (a is None) == (b is None)
        if a is not None:
            assert (a["donor"], a["receiver"]) == (b["donor"], b["receiver"])
            d = a["donor"]
            # the donor's bottom node as it was (the host loop's own "before" rows are views on CPU tensors: compared with the state instead)
            assert np.array_equal(a["before"][0], state["lb"][d, 0]) and np.array_equal(a["before"][1], state["ub"][d, 0])
            assert np.array_equal(a["before"][2], b["before"][2])
            for x, y in zip(a["after"], b["after"]):
                assert np.array_equal(x, y), case
            for x, y in zip(a["before"], a["after"]):
                assert np.array_equal(x, y), case


# ------------------------------------------------------------------------------------------------ the shape of the Interval forest drivers
def _sources():
    import os
    import pcp_amd
    root = os.path.dirname(os.path.abspath(pcp_amd.__file__))
    return {n: open(os.path.join(root, n)).read() for n in sorted(os.listdir(root)) if n.endswith(".py")}


def test_no_public_forest_driver_has_a_private_keyword():
    import inspect
    import pcp_amd.engine as E
    import pcp_amd.search_forest as SF
    public = [(f"Context.{n}", f) for n, f in vars(E.Context).items() if callable(f) and not n.startswith("_")]
    public += [(n, f) for n, f in vars(SF).items() if inspect.isfunction(f) and f.__module__ == SF.__name__ and not n.startswith("_")]
    assert len(public) > 40
    for name, fn in public:
        private = [p for p in inspect.signature(fn).parameters if p.startswith("_")]
        assert not private, (name, private)


def test_the_back_doors_are_gone_and_the_loop_is_called_from_one_place():
    import re
    src = _sources()
    # (as identifiers of their own: the entry point pcp_dfs_forest_device_neq_sink keeps its name)
    for word in ("_by_store", "_enum_entry", "_neq_sink", "_call=", "_obj="):
        assert not [n for n, s in src.items() if re.search(r"(?<![A-Za-z0-9])" + re.escape(word), s)], word
    assert src["engine.py"].count("run_forest_loop(") == 1


def test_grow_releases_each_old_array_before_it_allocates_the_next(monkeypatch):
    """The peak of ForestStacks.grow is one old array next to the new ones, not all the old ones: when the new ``ub`` is allocated the old
    ``lb`` is gone, and so on down the row arrays."""
    import weakref
    T, cap, V = 3, 2, 4
    z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype)
    fs = ForestStacks(z(T, cap, V), z(T, cap, V), z(T, cap, dtype=torch.uint8), torch.ones(T, dtype=torch.int32), z(T), z(T, 5, dtype=torch.int64), max_capacity=8,
                      dirty=z(T, cap), path=z(T, 1, 2), row_base=z(T, cap), row_excl=z(T, cap, 2), path_capacity=1)
    names = [n for n in ForestStacks.ROWS]
    old = {n: weakref.ref(getattr(fs, n)) for n in names}
    alive_at, rows = {}, ForestStacks.rows

    def watched(name, *a, **k):
        alive_at[name] = [n for n in names if old[n]() is not None]
        return rows(name, *a, **k)
    monkeypatch.setattr(ForestStacks, "rows", staticmethod(watched))
    assert fs.grow() and fs.capacity == 2 * cap
    for i, n in enumerate(names):
        assert alive_at[n] == names[i:], (n, alive_at[n])
    assert all(r() is None for r in old.values())
