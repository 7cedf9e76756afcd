"""The cases of the formula-store exclusion tests (test_form_excl_cpu.py, test_form_excl_gpu.py): pcp_propagate_device_form_excl — nodes of a
store WITH formula units (the schedules of form_forest_cases.py: tasks under propagators::Cumulative, optionally a makespan variable) that carry
value exclusions x != v of their own (Enumerate's right branches, enumerate.rs:54-59), optionally under branch and bound
(branch_and_bound.rs:64-84).  The judge of every node is the oracle on the store plus one XNeqY(x, Constant(v)) allocated behind it per entry
(Branch::distribute, branch.rs:36-55).  Every property a case is there for is asserted on the oracle here, when the case is built.
TEST INFRASTRUCTURE."""
import functools

import numpy as np

from oracle import oracle as orc
from pcp_amd import model as M

import form_forest_cases as FC
from small_excl_cases import NONE, csr, fold, units  # noqa: F401  (the 8-byte entries, the CSR and the fold are the small-store tests')

# the models of the SEARCH tests: form_forest_cases.MODELS, the windows narrowed where the Enumerate tree under MiddleVal would otherwise be too
# large for a test (name -> (durations, resources, start window, makespan window or None)); TREE_CEILING is a condition for test time
SEARCH_MODELS = {
    "A4": FC.MODELS["A4"],
    "C4mk": FC.MODELS["C4mk"],
    "D5mk": FC.MODELS["D5mk"],
}
TREE_CEILING = 20000


# ---------------------------------------------------------------------------------------------------------------- models
def build(durations, resources, win, mk_win):
    """form_forest_cases.schedule on explicit parameters: (vs, cs, index of the makespan variable or None)."""
    vs, cs = M.VStore(), M.CStore()
    starts = [vs.alloc(win) for _ in durations]
    mk = vs.alloc(mk_win) if mk_win else None
    cap = vs.alloc((FC.CAPACITY, FC.CAPACITY))
    M.Cumulative(starts, [M.Constant(d) for d in durations], [M.Constant(r) for r in resources], cap).join(vs, cs)
    if mk is not None:
        for s, d in zip(starts, durations):
            cs.alloc(M.x_leq_y(M.Addition(s, d), mk))
    return vs, cs, (mk.idx if mk is not None else None)


@functools.lru_cache(maxsize=None)
def store(name):
    """(vs, cs, mk, lb0, ub0, pushes, sums) of a model: a name of form_forest_cases.MODELS, "wide" (A4's tasks over starts 0 .. 100: room for
    the chain) or "search:<name>" (SEARCH_MODELS)."""
    if name == "wide":
        vs, cs, mk = build(*FC.MODELS["A4"][:2], (0, 100), None)
    elif name.startswith("search:"):
        vs, cs, mk = build(*SEARCH_MODELS[name[7:]])
    else:
        vs, cs, mk = FC.schedule(name)
    lb0, ub0 = vs.bounds()
    sums = []
    pushes = cs.pushes(len(vs), sums_out=sums)
    return vs, cs, mk, lb0, ub0, pushes, sums


def push(target, name, set_words=0):
    """The store on an engine Context or an OracleModel (model.push_model from the cached pushes)."""
    vs, _, _, _, _, pushes, sums = store(name)
    target.reset_model(len(vs), set_words)
    for members in sums:
        target.push_sum(members)
    for p in pushes:
        if p[0] == "props":
            target.push_props(p[1])
        else:
            target.push_formula(p[1], p[2])
    return len(vs)


# ---------------------------------------------------------------------------------------------------------------- the judge
_MODELS, _JUDGED = {}, {}


def model_with(name, ex=()):
    """The oracle model of the store plus XNeqY(x, Constant(v)) behind it per entry; one per distinct list."""
    key = (name, tuple(ex))
    if key not in _MODELS:
        om = orc.OracleModel(len(store(name)[0]))
        push(om, name)
        if ex:
            om.push_props(units(ex))
        if len(_MODELS) > 4096:  # (searches make many lists: keep the memory bounded, the plain models first in line to stay)
            for k in [k for k in _MODELS if k[1]][:2048]:
                del _MODELS[k]
        _MODELS[key] = om
    return _MODELS[key]


def judge(name, L, U, ex):
    """(status, lb, ub) of ONE node under the oracle; computed once per distinct node, shared and never changed."""
    ex = tuple((int(a), int(b)) for a, b in ex)
    key = (name, L.tobytes(), U.tobytes(), ex)
    if key not in _JUDGED:
        r = model_with(name, ex).consistency(L[None], U[None], None)
        _JUDGED[key] = (int(r[3][0]), r[0][0].copy(), r[1][0].copy())
    return _JUDGED[key]


def oracle_nodes(name, L, U, excl):
    """(lb, ub, status) of every node under the oracle, each with its own exclusions."""
    lb, ub, st = L.copy(), U.copy(), np.zeros(len(L), np.uint8)
    for i in range(len(L)):
        st[i], lb[i], ub[i] = judge(name, L[i], U[i], excl[i])
    return lb, ub, st


def bnb_expected(name, L, U, excl, var, mode, best):
    """What pcp_propagate_device_form_excl leaves with an objective: (lb, ub, status, emptied, best, improved, winner or None) — the fold
    (small_excl_cases.fold: an emptied node keeps its row and is False), the judge, the reduce (the first of equal values wins)."""
    lb, ub, st, emp = L.copy(), U.copy(), np.zeros(len(L), np.uint8), np.zeros(len(L), bool)
    for i in range(len(L)):
        fl, fu, emp[i] = fold(L[i], U[i], var, mode, best)
        if not emp[i]:
            st[i], lb[i], ub[i] = judge(name, fl, fu, excl[i])
    true = np.nonzero(st == 1)[0]
    win = None
    if len(true):
        vals = lb[true, var].astype(np.int64)
        w = int(true[vals.argmin() if mode == "min" else vals.argmax()])
        if (lb[w, var] < best) if mode == "min" else (lb[w, var] > best):
            win = w
    return lb, ub, st, emp, (int(lb[win, var]) if win is not None else best), (1 if win is not None else 0), win


@functools.lru_cache(maxsize=None)
def records(name, limit=400):
    """The first nodes of the oracle's own DFS (BinarySplit) over the store: the record dict of OracleModel.search."""
    _, _, _, lb0, ub0, _, _ = store(name)
    return model_with(name).search(lb0, ub0, all_solutions=True, node_limit=limit, max_records=limit)[2]


# ---------------------------------------------------------------------------------------------------------------- per-entry cases
ENTRY_KINDS = ("none", "at_lb", "at_ub", "interior", "outside", "assigned_same", "assigned_other", "dup", "two_empty", "badvar")


@functools.lru_cache(maxsize=None)
def entry_cases():
    """One node per kind on A4: (name, L, U, excl, kinds).  Rows are the root with one start narrowed, so that the entry meets the domain the
    kind asks for; what each kind has to show is asserted here on the oracle."""
    name = "A4"
    vs, _, _, lb0, ub0, _, _ = store(name)
    n = len(vs)

    def row(x=None, lo=None, hi=None):
        l, u = lb0.copy(), ub0.copy()
        if x is not None:
            l[x], u[x] = lo, hi
        return l, u

    nodes = {
        "none": (row(), []),
        "at_lb": (row(), [(1, 0)]),
        "at_ub": (row(), [(2, 5)]),
        "interior": (row(), [(1, 2)]),
        "outside": (row(), [(3, 9), (3, -2)]),
        "assigned_same": (row(3, 4, 4), [(3, 4)]),
        "assigned_other": (row(3, 4, 4), [(3, 3)]),
        "dup": (row(), [(1, 0), (1, 0), (1, 5), (1, 0)]),
        "two_empty": (row(2, 2, 3), [(2, 2), (2, 3)]),
        "badvar": (row(), [(1, 0), (n, 3)]),
    }
    L = np.stack([nodes[k][0][0] for k in ENTRY_KINDS])
    U = np.stack([nodes[k][0][1] for k in ENTRY_KINDS])
    excl = [nodes[k][1] for k in ENTRY_KINDS]
    kinds = np.array(ENTRY_KINDS)
    ok = kinds != "badvar"
    base = oracle_nodes(name, L[ok], U[ok], [[] for _ in range(int(ok.sum()))])
    ref = oracle_nodes(name, L[ok], U[ok], [e for e, o in zip(excl, ok) if o])
    at = {k: i for i, k in enumerate(kinds[ok])}
    assert base[2][at["none"]] == 2
    assert ref[2][at["at_lb"]] != 0 and ref[0][at["at_lb"]][1] >= 1 and base[0][at["at_lb"]][1] == 0          # the value at the lower bound goes
    assert ref[2][at["at_ub"]] != 0 and ref[1][at["at_ub"]][2] <= 4 and base[1][at["at_ub"]][2] == 5          # ... at the upper bound
    i = at["interior"]                                                                                          # inside: nothing moves, Unknown
    assert ref[2][i] == 2 and np.array_equal(ref[0][i], base[0][i]) and np.array_equal(ref[1][i], base[1][i])
    i = at["outside"]                                                                                           # entailed from the start
    assert ref[2][i] == base[2][i] and np.array_equal(ref[0][i], base[0][i]) and np.array_equal(ref[1][i], base[1][i])
    assert ref[2][at["assigned_same"]] == 0 and base[2][at["assigned_same"]] != 0                               # x assigned to the value: False
    i = at["assigned_other"]
    assert ref[2][i] == base[2][i] != 0 and np.array_equal(ref[0][i], base[0][i])
    i = at["dup"]
    assert ref[2][i] != 0 and ref[0][i][1] >= 1 and ref[1][i][1] <= 4
    assert ref[2][at["two_empty"]] == 0 and base[2][at["two_empty"]] != 0                                       # the two values of a two-value domain
    return name, L, U, excl, kinds


# ---------------------------------------------------------------------------------------------------------------- interplay
@functools.lru_cache(maxsize=None)
def interplay_cases():
    """{name: (L, U, excl, tags)} — nodes where exclusions and formula units need each other, found among the nodes of the oracle's DFS and
    asserted on the oracle:
      a: an exclusion narrows a start at a bound (its domain keeps a value), and what the units make of that fails the node;
      b: the entry's value is INSIDE its variable's domain on entry, the units alone bring a bound onto it, and with the entry the bound moves
         past it (the exclusion removes it in a later round);
      c: every unit is entailed (the node is True without its list) and one entry is open: Unknown."""
    out = {}
    for name in ("A4", "C4mk"):
        vs, _, mk, _, _, _, _ = store(name)
        n_tasks = len(FC.MODELS[name][0])
        rec = records(name)
        L, U, excl, tags = [], [], [], []
        want = {"a": 2, "b": 2}
        for i in range(len(rec["status"])):
            li, ui, lo, uo, st = rec["lb_in"][i], rec["ub_in"][i], rec["lb_out"][i], rec["ub_out"][i], int(rec["status"][i])
            if st == 2 and want["a"]:
                for x in range(n_tasks):
                    for v, keep in ((int(lo[x]), uo[x] > lo[x]), (int(uo[x]), uo[x] > lo[x])):
                        if keep and want["a"] and judge(name, lo, uo, [(x, v)])[0] == 0:
                            L.append(lo); U.append(uo); excl.append([(x, v)]); tags.append("a")
                            want["a"] -= 1
            if st == 2 and want["b"]:
                for x in range(n_tasks):
                    for v, moved in ((int(lo[x]), lo[x] > li[x]), (int(uo[x]), uo[x] < ui[x])):
                        if not (moved and li[x] < v < ui[x] and lo[x] < uo[x] and want["b"]):
                            continue
                        s, l2, u2 = judge(name, li, ui, [(x, v)])
                        if s != 0 and not (l2[x] <= v <= u2[x]):
                            L.append(li); U.append(ui); excl.append([(x, v)]); tags.append("b")
                            want["b"] -= 1
        assert not want["a"] and not want["b"], (name, want)
        if mk is not None:  # c: a schedule with its makespan variable still open
            sol = np.nonzero((rec["status"] == 1) & (rec["ub_out"][:, mk] - rec["lb_out"][:, mk] >= 2))[0]
            assert len(sol), name
            lo, uo = rec["lb_out"][sol[0]], rec["ub_out"][sol[0]]
            assert judge(name, lo, uo, [])[0] == 1
            ex = [(mk, int(lo[mk]) + 1)]
            s, l2, u2 = judge(name, lo, uo, ex)
            assert s == 2 and np.array_equal(l2, lo) and np.array_equal(u2, uo)
            L.append(lo); U.append(uo); excl.append(ex); tags.append("c")
        out[name] = (np.stack(L), np.stack(U), excl, np.array(tags))
    assert "c" in out["C4mk"][3]
    return out


# ---------------------------------------------------------------------------------------------------------------- the chain, many units
CHAIN = 70


@functools.lru_cache(maxsize=None)
def chain_cases():
    """("wide", L, U, excl, index of the chain): 70 consecutive values from the lower bound of start 1, shuffled, in ONE list of more than 64
    entries — they only ever fall one at a time; next to it the same node with lists of 0, 1, 64 and 65 seeded entries around the bounds."""
    name = "wide"
    _, _, _, lb0, ub0, _, _ = store(name)
    rng = np.random.default_rng(4802)
    excl = []
    for c in (0, 1, 64, 65):
        xs = rng.integers(0, 4, c)
        vals = np.where(rng.random(c) < 0.5, rng.integers(-1, 5, c), rng.integers(96, 103, c))
        excl.append([(int(a), int(b)) for a, b in zip(xs, vals)])
    excl.append([(1, int(v)) for v in rng.permutation(np.arange(0, CHAIN))])
    L, U = np.tile(lb0, (len(excl), 1)), np.tile(ub0, (len(excl), 1))
    chain = len(excl) - 1
    assert len(excl[chain]) == CHAIN > 64
    st, lb, ub = judge(name, L[chain], U[chain], excl[chain])
    assert st == 2 and lb[1] == CHAIN
    return name, L, U, excl, chain


@functools.lru_cache(maxsize=None)
def many_unit_cases():
    """("six", L, U, excl): a store of more than 64 units — a lane runs two of them — on Unknown nodes of its DFS, with entries at the bounds
    of every open start."""
    name = "six"
    om = model_with(name)
    assert om.n_units > 64, om.n_units
    rec = records(name, 60)
    unk = np.nonzero(rec["status"] == 2)[0][:8]
    L, U = np.ascontiguousarray(rec["lb_out"][unk]), np.ascontiguousarray(rec["ub_out"][unk])
    excl = []
    for i in range(len(L)):
        open_ = [x for x in range(6) if U[i, x] > L[i, x]]
        excl.append([(x, int(b)) for x in open_ for b in ((L[i, x], U[i, x]) if i % 2 else (L[i, x],))])
    ref, base = oracle_nodes(name, L, U, excl), oracle_nodes(name, L, U, [[] for _ in excl])
    assert not (np.array_equal(ref[2], base[2]) and np.array_equal(ref[0], base[0]) and np.array_equal(ref[1], base[1]))
    return name, L, U, excl


# ---------------------------------------------------------------------------------------------------------------- branch and bound
@functools.lru_cache(maxsize=None)
def bnb_batch():
    """("C4mk", L, U, excl, var, tie): Unknown nodes of the store's DFS, two schedules of the same makespan `tie` in the middle (rows 3 and 4),
    Unknown nodes again; three nodes carry exclusions."""
    name = "C4mk"
    _, _, mk, _, _, _, _ = store(name)
    rec = records(name)
    unk, sol = np.nonzero(rec["status"] == 2)[0], np.nonzero(rec["status"] == 1)[0]
    spans = rec["lb_out"][sol, mk]
    tie = next(int(v) for v in spans if (spans == v).sum() >= 2)
    two = sol[spans == tie][:2]
    assert not np.array_equal(rec["lb_out"][two[0]], rec["lb_out"][two[1]])
    pick = np.concatenate([unk[:3], two, unk[3:6]])
    L, U = np.ascontiguousarray(rec["lb_out"][pick]), np.ascontiguousarray(rec["ub_out"][pick])
    excl = [[] for _ in range(len(L))]
    for i in (1, 5, 7):
        x = int(np.nonzero(U[i] > L[i])[0][0])
        excl[i] = [(x, int(L[i, x])), (x, int(U[i, x]))]
    return name, L, U, excl, mk, tie


BNB_KINDS = ("none", "above", "tie", "below")


def bnb_best(mode, kind, tie):
    """The incumbent of a case: none, above every node, equal to the makespan of the two schedules that tie, below every node."""
    return {"none": NONE[mode], "above": 14, "tie": tie, "below": -1}[kind]


def bnb_bests(tie):
    """(mode, incumbent) of every case, in both modes."""
    return [(m, bnb_best(m, k, tie)) for m in ("min", "max") for k in BNB_KINDS]


# ---------------------------------------------------------------------------------------------------------------- all solutions
@functools.lru_cache(maxsize=None)
def all_schedules(name):
    """Every assignment of the start times of SEARCH_MODELS[name] that is a schedule, by trying them all (a model without a makespan variable)."""
    import itertools
    durations, resources, win, mk_win = SEARCH_MODELS[name]
    assert mk_win is None
    out = set()
    for s in itertools.product(range(win[0], win[1] + 1), repeat=len(durations)):
        if all(sum(r for si, d, r in zip(s, durations, resources) if si <= t < si + d) <= FC.CAPACITY for t in range(win[0], win[1] + max(durations) + 1)):
            out.add(s)
    return frozenset(out)


def covered(n_tasks, boxes):
    """The start-time assignments inside the (lb, ub) rows of Satisfiable nodes, and how many the boxes hold in all (equal: no two overlap).
    In interval mode a node is Satisfiable as soon as every unit is entailed — its starts need not be assigned, so one node stands for every
    assignment in its box, and two distributors cut the same solutions into different boxes."""
    import itertools
    out, total = set(), 0
    for l, u in boxes:
        pts = list(itertools.product(*[range(int(a), int(b) + 1) for a, b in zip(l[:n_tasks], u[:n_tasks])]))
        total += len(pts)
        out |= set(pts)
    return out, total
