"""pcp_dfs_forest_steal on the device (pcp_steal.hip) through Context.forest_steal, on synthetic forest states — no search is involved: the entry
works on the state alone, so a context of n_vars plain variables and one propagator is enough.  Every result is compared with
forest_steal_cases.steal_reference, the contract restated in numpy: done, sp, the rows [0, sp) of lb, ub, dirty, row_base and row_excl, the
path entries [0, row_base[t][0]), a donor's whole path, and every tree in no valid pair bit for bit."""
import numpy as np
import pytest

import forest_steal_cases as FC
from pcp_amd import model as M

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 4, 63, 64, 65, 257, 1000]  # scalar and 16-byte paths, a slice seam (64 threads a slice), more than one slice
ERR_ARG = -1


@pytest.fixture(scope="module")
def contexts():
    import pcp_amd.engine as E
    made = {}

    def get(V, set_words=0):
        if (V, set_words) not in made:
            c = E.Context(0)
            c.set_model(V, M.lower_units([M.XNeqY(M.Identity(0), M.Constant(5))], V), set_words=set_words)
            if set_words:
                c.set_hull(0, 63)
            made[(V, set_words)] = c
        return made[(V, set_words)]

    yield get
    for c in made.values():
        c.close()


class OnDevice:
    """A state's arrays as device tensors and the structs over them."""

    def __init__(self, ctx, state, misalign=False, null_path=False, null_dirty=False):
        import torch
        import pcp_amd.engine as E
        self.torch, self.ctx, self.state = torch, ctx, state
        dev = torch.device("cuda", ctx.device)
        self.t = {}
        for name in FC.ARRAYS:
            a = state[name]
            if a is None:
                self.t[name] = None
            elif misalign and name in ("lb", "ub"):  # rows that start one word behind a 16-byte boundary
                flat = torch.zeros(a.size + 1, dtype=torch.int32, device=dev)
                flat[1:] = torch.from_numpy(a.reshape(-1)).to(dev)
                self.t[name] = flat[1:].reshape(a.shape)
                assert self.t[name].data_ptr() % 16 == 4
            else:
                self.t[name] = torch.from_numpy(a.copy()).to(dev)
        p = lambda x: None if x is None else x.data_ptr()
        t = self.t
        self.st = E.DfsState(p(t["lb"]), p(t["ub"]), state["capacity"], p(t["sp"]), None, None, None, None, None if null_dirty else p(t["dirty"]))
        self.ex = None
        if state["row_base"] is not None:
            self.ex = E.ForestExcl(None if null_path else p(t["path"]), p(t["row_base"]), p(t["row_excl"]), state["path_capacity"], 0)
        self.T = len(state["sp"])

    def steal(self, pairs, n_trees=None):
        torch = self.torch
        dev = self.t["sp"].device
        pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        d_pairs = torch.from_numpy((pairs & 0xFFFFFFFF).astype(np.uint32).view(np.int32).copy()).to(dev)
        done = torch.full((len(pairs),), 77, dtype=torch.int32, device=dev)
        self.ctx.forest_steal(self.st, self.T if n_trees is None else n_trees, self.ex, d_pairs, done)
        torch.cuda.synchronize()
        return self.download(), done.cpu().numpy()

    def download(self):
        got = FC.copy_state(self.state)
        for name in FC.ARRAYS:
            if self.t[name] is not None:
                got[name] = self.t[name].cpu().numpy()
        return got


def check(ctx, state, pairs, what="", **how):
    want, done_want = FC.steal_reference(state, pairs)
    got, done_got = OnDevice(ctx, state, **how).steal(pairs)
    FC.assert_steal_matches(state, want, got, pairs, done_want, done_got, what=what)
    return done_want


def planner_pairs(sp, n):
    import torch
    from pcp_amd.search_forest import plan_steal_pairs
    return plan_steal_pairs(torch.from_numpy(np.asarray(sp, np.int32)), n).numpy()


@pytest.mark.parametrize("V", WIDTHS)
@pytest.mark.parametrize("excl", [False, True], ids=["split", "enum"])
def test_row_widths(contexts, V, excl):
    rng = np.random.default_rng(1000 + V + excl)
    sp = [5, 0, 2, 0, 3, 1, 0, 4, 0]
    state = FC.random_state(rng, len(sp), 5, V, sp=sp, excl=excl)
    done = check(contexts(V), state, planner_pairs(sp, len(sp)), what=("width", V))
    assert done.sum() == 4  # the trees with 5, 4, 3 and 2 rows each give one to the first four idle trees


@pytest.mark.parametrize("V,cap,rows", [(3, 2, 2), (4, 2, 2), (65, 5, 5), (64, 5, 5), (65, 300, 299), (64, 300, 299), (4, 300, 300), (1, 20, 9), (8, 20, 10)])
def test_stack_depths(contexts, V, cap, rows):
    """The smallest shift (one row), a full stack, many rows; 9 and 10 rows sit on either side of the move loop's unrolled body."""
    rng = np.random.default_rng(V * 1000 + rows)
    sp = [0, rows, 1, 0, rows]
    state = FC.random_state(rng, len(sp), cap, V, sp=sp)
    assert check(contexts(V), state, [(1, 0), (4, 3)], what=("depth", V, cap, rows)).sum() == 2


def test_misaligned_base_takes_the_word_path(contexts):
    rng = np.random.default_rng(5)
    sp = [0, 12, 3, 0]
    state = FC.random_state(rng, len(sp), 16, 64, sp=sp)
    assert check(contexts(64), state, [(1, 0), (2, 3)], misalign=True).sum() == 2


@pytest.mark.parametrize("dirty", [True, False], ids=["dirty", "no_dirty"])
def test_binary_split_state(contexts, dirty):
    rng = np.random.default_rng(11)
    sp = [3, 0, 0, 7, 1]
    state = FC.random_state(rng, len(sp), 8, 10, sp=sp, dirty=dirty, excl=False)
    assert check(contexts(10), state, [(3, 1), (0, 2)]).sum() == 2


def test_dirty_rows_ignored_when_the_state_has_none(contexts):
    """st->dirty == NULL: a buffer the caller keeps next to the state is not the entry's to move."""
    rng = np.random.default_rng(12)
    sp = [3, 0]
    state = FC.random_state(rng, 2, 4, 10, sp=sp, dirty=True, excl=False)
    dev = OnDevice(contexts(10), state, null_dirty=True)
    got, done = dev.steal([(0, 1)])
    assert done.tolist() == [1] and got["sp"].tolist() == [2, 1]
    assert np.array_equal(got["dirty"], state["dirty"])


@pytest.mark.parametrize("own", [False, True], ids=["no_entry", "entry"])
@pytest.mark.parametrize("nb", ["zero", "one", "full"])
def test_exclusion_prefix(contexts, nb, own):
    rng = np.random.default_rng(21)
    pc = 6
    sp = [4, 0, 2, 0]
    state = FC.random_state(rng, len(sp), 6, 7, sp=sp, path_capacity=pc)
    n = {"zero": 0, "one": 1, "full": pc}[nb]
    for d in (0, 2):
        state["row_base"][d, 0] = n
        state["row_base"][d, 1:sp[d]] = np.maximum(state["row_base"][d, 1:sp[d]], n)
        state["row_excl"][d, 0] = (3, -44) if own else (-1, 0)
    check(contexts(7), state, [(0, 1), (2, 3)], what=("prefix", nb, own))


def test_no_path_at_all(contexts):
    """path_capacity = 0 with path = NULL: every row_base is 0, the rows' own entries still move."""
    rng = np.random.default_rng(22)
    sp = [4, 0, 2, 0]
    state = FC.random_state(rng, len(sp), 6, 7, sp=sp, path_capacity=0)
    for t, n in enumerate(sp):
        state["row_base"][t, :n] = 0
    want, done_want = FC.steal_reference(state, [(0, 1), (2, 3)])
    got, done = OnDevice(contexts(7), state, null_path=True).steal([(0, 1), (2, 3)])
    FC.assert_steal_matches(state, want, got, [(0, 1), (2, 3)], done_want, done)
    assert done.tolist() == [1, 1]


# tree 0: 4 rows, 1: idle, 2: one row, 3: idle, 4: 3 rows, 5: idle, 6: more rows than the capacity, 7: a row_base beyond the path
BASE_SP = [4, 0, 1, 0, 3, 0, 9, 2]
INVALID = {
    "receiver_has_a_row": (0, 2),
    "donor_idle": (1, 3),
    "donor_one_row": (2, 3),
    "donor_over_capacity": (6, 3),
    "same_tree": (0, 0),
    "same_idle_tree": (1, 1),
    "donor_is_n_trees": (8, 1),
    "receiver_is_n_trees": (0, 8),
    "donor_all_ones": (0xFFFFFFFF, 1),
    "receiver_all_ones": (0, 0xFFFFFFFF),
    "row_base_beyond_path": (7, 3),
}


def invalid_state():
    rng = np.random.default_rng(31)
    state = FC.random_state(rng, len(BASE_SP), 6, 5, sp=BASE_SP, path_capacity=4)
    state["row_base"][7, :2] = 5  # path_capacity + 1
    return state


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_pair_alone(contexts, name):
    state = invalid_state()
    done = check(contexts(5), state, [INVALID[name]], what=name)
    assert done.tolist() == [0]


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_pair_next_to_valid_ones(contexts, name):
    state = invalid_state()
    bad = INVALID[name]
    # the valid pairs use trees 4 -> 5 only, so that no tree of the invalid pair is in a valid one twice
    for pairs in ([bad, (4, 5)], [(4, 5), bad], [bad, (4, 5), bad]):
        done = check(contexts(5), state, pairs, what=(name, pairs))
        assert done.tolist() == [1 if p == (4, 5) else 0 for p in pairs]


def test_all_invalid_pairs_in_one_call(contexts):
    state = invalid_state()
    pairs = [INVALID[k] for k in sorted(INVALID)] + [(4, 5)]
    done = check(contexts(5), state, pairs)
    assert done.tolist() == [0] * len(INVALID) + [1]


@pytest.mark.parametrize("order", ["valid_first", "valid_last"])
def test_verdict_is_on_the_state_before_the_call(contexts, order):
    """A idle, B with two rows: (B, A) is valid; (A, B) is not — and must not become so whatever the first pair has done by then."""
    rng = np.random.default_rng(41)
    A, B = 0, 1
    state = FC.random_state(rng, 3, 4, 9, sp=[0, 2, 1])
    pairs = [(B, A), (A, B)] if order == "valid_first" else [(A, B), (B, A)]
    done = check(contexts(9), state, pairs, what=order)
    assert done.tolist() == ([1, 0] if order == "valid_first" else [0, 1])


def test_more_pairs_than_compute_units(contexts):
    rng = np.random.default_rng(51)
    T = 600
    sp = np.zeros(T, np.int32)
    sp[::2] = rng.integers(2, 7, size=T // 2)
    state = FC.random_state(rng, T, 6, 65, sp=sp)
    pairs = [(2 * i, 2 * i + 1) for i in range(T // 2)]
    rng.shuffle(pairs)
    assert check(contexts(65), state, pairs).sum() == 300


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planner_shaped_input(contexts, seed):
    """n_pairs = T with the planner's pairs on a random sp: most pairs are invalid, and a tree of a valid pair is also in invalid ones."""
    rng = np.random.default_rng(60 + seed)
    T = 97
    state = FC.random_state(rng, T, 7, 12, path_capacity=5)
    pairs = planner_pairs(state["sp"], T)
    done = check(contexts(12), state, pairs, what=("planner", seed))
    donors, idle = FC.host_policy(state["sp"])
    assert done.sum() == min(len(donors), len(idle)) and 0 < done.sum() < T


def test_no_pairs_is_ok(contexts):
    rng = np.random.default_rng(70)
    state = FC.random_state(rng, 3, 4, 5, sp=[3, 0, 0])
    dev = OnDevice(contexts(5), state)
    dev.ctx.forest_steal(dev.st, 3, dev.ex, None, None, n_pairs=0)
    dev.torch.cuda.synchronize()
    got = dev.download()
    for name in FC.ARRAYS:
        assert np.array_equal(got[name], state[name]), name


def test_refusals(contexts):
    import torch
    import pcp_amd.engine as E
    rng = np.random.default_rng(71)
    state = FC.random_state(rng, 3, 4, 5, sp=[3, 0, 0], path_capacity=3)
    ctx = contexts(5)
    dev = OnDevice(ctx, state)
    cuda = dev.t["sp"].device
    pairs = torch.tensor([[0, 1]], dtype=torch.int32, device=cuda)
    done = torch.full((1,), 77, dtype=torch.int32, device=cuda)
    base = dict(lb=dev.st.lb, ub=dev.st.ub, capacity=4, sp=dev.st.sp, dirty=dev.st.dirty)
    st_with = lambda **kw: E.DfsState(**{**base, **kw})
    ex_base = dict(path=dev.ex.path, row_base=dev.ex.row_base, row_excl=dev.ex.row_excl, path_capacity=3, val=0)
    ex_with = lambda **kw: E.ForestExcl(**{**ex_base, **kw})
    cases = {
        "null_state": lambda: ctx.forest_steal(None, 3, dev.ex, pairs, done),
        "null_lb": lambda: ctx.forest_steal(st_with(lb=None), 3, dev.ex, pairs, done),
        "null_ub": lambda: ctx.forest_steal(st_with(ub=None), 3, dev.ex, pairs, done),
        "null_sp": lambda: ctx.forest_steal(st_with(sp=None), 3, dev.ex, pairs, done),
        "null_pairs": lambda: ctx.forest_steal(dev.st, 3, dev.ex, None, done, n_pairs=1),
        "null_done": lambda: ctx.forest_steal(dev.st, 3, dev.ex, pairs, None),
        "no_trees": lambda: ctx.forest_steal(dev.st, 0, dev.ex, pairs, done),
        "capacity_1": lambda: ctx.forest_steal(st_with(capacity=1), 3, dev.ex, pairs, done),
        "null_row_base": lambda: ctx.forest_steal(dev.st, 3, ex_with(row_base=None), pairs, done),
        "null_row_excl": lambda: ctx.forest_steal(dev.st, 3, ex_with(row_excl=None), pairs, done),
        "null_path": lambda: ctx.forest_steal(dev.st, 3, ex_with(path=None), pairs, done),
        "set_mode": lambda: contexts(5, set_words=1).forest_steal(dev.st, 3, dev.ex, pairs, done),
    }
    for name, call in cases.items():
        with pytest.raises(E.PcpError) as e:
            call()
        assert e.value.code == ERR_ARG, name
        if name == "set_mode":
            assert "pcp_dfs_forest_split_set" in str(e.value)
    torch.cuda.synchronize()
    got = dev.download()
    for name in FC.ARRAYS:
        assert np.array_equal(got[name], state[name]), name
    assert done.cpu().tolist() == [77]  # nothing was launched
    # and the same call without a defect runs
    ctx.forest_steal(dev.st, 3, dev.ex, pairs, done)
    torch.cuda.synchronize()
    assert done.cpu().tolist() == [1] and dev.download()["sp"].tolist() == [2, 1, 0]
