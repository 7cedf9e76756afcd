"""Shared cases of the formula-leaf parity tests (test_formula_leaf_cpu.py, test_formula_leaf_gpu.py): what the formula kernels' own
is_subsumed() of every leaf kind (rec_subsumed in pcp_formula.hpp, rec_subsumed_set in pcp_setform.hpp) decides, on stores the older
generators never draw.

(a) Exhaustive Kleene tables: one leaf under a guard g in (0, 1), every box of the operands over a tiny signed domain, crossed with the
    guard open, 0 and 1.  Three stores of one unit each per leaf variant (FORMS):
      or_g      Or((leaf, Boolean(g)))       g = 0 propagates the leaf, g = 1 entails the unit
      or_not_g  Or((leaf, BooleanNeg(g)))    the same with the guard's sense reversed
      equiv     equivalence(Boolean(g), leaf), for the kinds whose not_ the mirror implements: the De Morgan negation of the leaf.
(b) Random stores over every kind, satisfied by a planted assignment, on positive, zero-crossing and negative domains, with up to 130
    units and 70 variables, and their nodes and `active` rows.
(c) Mask edges of the unit step: units of exactly 64 tree nodes, a flat Conjunction of 67, and a unit of 65 nodes that is not flat.

The oracle's answers are computed once per process and never modified.  Boolean / BooleanNeg over an Addition view are accepted by the
mirror (an Elementary over any view) and by both lowerings, so their tables are in — without the boxes on which the reference panics:
Boolean::propagate on a domain of several values without the one it assigns is a non-monotonic update (boolean.rs:132-134,
variable/store.rs:153-156; the oracle raises OraclePanic there), so such a domain holds the values the table's leaves assign."""
import functools

import numpy as np

from oracle import oracle as orc
from pcp_amd import model as M

from test_set_mode import random_sets
from util import random_active, splitmix64

FORMS = ("or_g", "or_not_g", "equiv")
GUARDS = ((0, 1), (0, 0), (1, 1))
D = (-2, 2)


def oracle_model(vs, cs):
    om = orc.OracleModel(len(vs))
    M.push_model(om, cs, len(vs))
    return om


def frozen(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------------------- (a) Kleene tables
def sub_intervals(lo, hi):
    return [(a, b) for a in range(lo, hi + 1) for b in range(a, hi + 1)]


def subsets(lo, hi):
    vals = list(range(lo, hi + 1))
    return [tuple(v for k, v in enumerate(vals) if (m >> k) & 1) for m in range(1, 1 << len(vals))]


def _variants():
    """name -> (operand domains, leaf builder over the operand views, whether not_ is implemented, interval mode only)."""
    v = {}
    for off in (-1, 0, 2):
        v[f"NEQ{off:+d}"] = ([D, D], lambda o, off=off: M.XNeqY(o[0], M.Addition(o[1], off)), True, False)
        v[f"EQ{off:+d}"] = ([D, D], lambda o, off=off: M.XEqY(o[0], M.Addition(o[1], off)), True, False)
        v[f"LT{off:+d}"] = ([D, D], lambda o, off=off: M.XLessY(o[0], M.Addition(o[1], off)), True, False)
    v["LTconst"] = ([D], lambda o: M.XLessY(o[0], M.Constant(0)), True, False)
    v["LTsum"] = ([D, D, D], lambda o: M.XLessY(o[0], M.Sum((o[1], o[2]))), True, True)
    v["LT3+1"] = ([D, D, D], lambda o: M.XLessYPlusZ(o[0], o[1], M.Addition(o[2], 1)), True, False)
    v["GT3"] = ([D, D, D], lambda o: M.XGreaterYPlusZ(o[0], o[1], o[2]), True, False)
    for off in (-1, 0, 1):
        v[f"EQ3{off:+d}"] = ([D, D, D], lambda o, off=off: M.XEqYPlusZ(o[0], o[1], M.Addition(o[2], off)), False, False)
    v["BOOL-2"] = ([(1, 4)], lambda o: M.Boolean(M.Addition(o[0], -2)), True, False)
    v["NBOOL-2"] = ([(1, 4)], lambda o: M.BooleanNeg(M.Addition(o[0], -2)), True, False)
    # non-negative factors only: the oracle's product over negative factors is not pinned against the reference (test_mul3_with_addition_views)
    v["MUL3"] = ([(-2, 6), (0, 3), (0, 2)], lambda o: M.XEqYMulZ(o[0], o[1], M.Addition(o[2], 1)), False, True)
    return v


VARIANTS = _variants()
INTERVAL_TABLES = [(n, f) for n, (_, _, neg, _) in VARIANTS.items() for f in FORMS if neg or f != "equiv"]
SET_TABLES = [(n, f) for n, f in INTERVAL_TABLES if not VARIANTS[n][3]]
SET_LAYOUTS = ((1, -2), (2, -64))  # (set_words, base): one word from -2; two words with -1 = bit 63 of word 0 and 0 = bit 0 of word 1


def _assigned_values(name, form):
    """The values of b that Boolean / BooleanNeg over Addition(b, -2) assign in this table: 3, 2, or both (the equivalence negates the
    leaf).  A domain of several values must hold them (the module docstring); None for the other kinds."""
    if "BOOL" not in name:
        return None
    return {2, 3} if form == "equiv" else ({3} if name.startswith("BOOL") else {2})


def table_store(name, form):
    """(vs, cs, number of operands): the operands, then the guard."""
    doms, build, _, _ = VARIANTS[name]
    vs, cs = M.VStore(), M.CStore()
    ops = [vs.alloc(d) for d in doms]
    g = vs.alloc((0, 1))
    leaf = build(ops)
    if form == "or_g":
        cs.alloc(M.Or((leaf, M.Boolean(g))))
    elif form == "or_not_g":
        cs.alloc(M.Or((leaf, M.BooleanNeg(g))))
    else:
        cs.alloc(M.equivalence(M.Boolean(g), leaf))
    return vs, cs, len(doms)


def _cross(choices):
    """Every combination of one row of each choices[i] ([n_i, ...]): index arrays [n_nodes] per operand."""
    grids = np.meshgrid(*[np.arange(len(c)) for c in choices], indexing="ij")
    return [g.reshape(-1) for g in grids]


@functools.lru_cache(maxsize=None)
def interval_table(name, form):
    """(vs, cs, L, U, open): every box of the operands x the three guard states (guard-major); `open` marks the nodes whose guard is (0, 1)."""
    vs, cs, k = table_store(name, form)
    need = _assigned_values(name, form)
    boxes = [np.array([(a, b) for a, b in sub_intervals(*d) if need is None or a == b or need <= set(range(a, b + 1))], np.int32)
             for d in VARIANTS[name][0]] + [np.array(GUARDS, np.int32)]
    idx = _cross([boxes[-1]] + boxes[:-1])  # the guard varies slowest
    idx = idx[1:] + idx[:1]
    L = np.stack([b[i, 0] for b, i in zip(boxes, idx)], axis=1).astype(np.int32)
    U = np.stack([b[i, 1] for b, i in zip(boxes, idx)], axis=1).astype(np.int32)
    return (vs, cs) + frozen((L, U, idx[-1] == 0))


@functools.lru_cache(maxsize=None)
def interval_table_reference(name, form):
    vs, cs, L, U, _ = interval_table(name, form)
    return frozen(oracle_model(vs, cs).consistency(L, U, None)[:4])


def _words(values, sw, base):
    w = np.zeros(sw, np.uint64)
    for v in values:
        w[(v - base) >> 6] |= np.uint64(1) << np.uint64((v - base) & 63)
    return w


@functools.lru_cache(maxsize=None)
def set_table(name, form, sw, base):
    """(vs, cs, bits [n, V, sw], open).  Kinds of one or two operands: every non-empty subset of each operand's domain; three operands:
    every interval box, and the same boxes with the middle value of x removed (x of three values or more)."""
    vs, cs, k = table_store(name, form)
    doms = VARIANTS[name][0]
    need = _assigned_values(name, form)
    if k <= 2:
        choices = [[c for c in subsets(*d) if need is None or len(c) == 1 or need <= set(c)] for d in doms]
    else:
        choices = [[tuple(range(a, b + 1)) for a, b in sub_intervals(*d)] for d in doms]
        choices[0] = choices[0] + [tuple(v for v in c if v != (c[0] + c[-1]) // 2) for c in choices[0] if len(c) >= 3]
    choices.append([(0, 1), (0,), (1,)])
    words = [np.stack([_words(c, sw, base) for c in ch]) for ch in choices]
    idx = _cross([words[-1]] + words[:-1])
    idx = idx[1:] + idx[:1]
    bits = np.stack([w[i] for w, i in zip(words, idx)], axis=1)
    return (vs, cs) + frozen((bits, idx[-1] == 0))


@functools.lru_cache(maxsize=None)
def set_table_reference(name, form, sw, base):
    vs, cs, bits, _ = set_table(name, form, sw, base)
    return frozen(oracle_model(vs, cs).consistency_set(bits, base, None)[:5])


def table_counts(rows_in, rows_out, status, open_):
    """The five figures of one table.  Guard open: nodes that end True, nodes that end with the guard assigned (not failed), nodes left
    unchanged (not failed).  Guard closed: nodes whose operands were narrowed (not failed), nodes that failed.  rows_*: [n, V] + any
    trailing axes (bounds stacked as [n, V, 2], or bit words), the guard is the last variable."""
    n = len(status)
    rin, rout = rows_in.reshape(n, rows_in.shape[1], -1), rows_out.reshape(n, rows_out.shape[1], -1)
    alive = status != M.FALSE
    g_moved = (rin[:, -1] != rout[:, -1]).any(axis=1)
    ops_moved = (rin[:, :-1] != rout[:, :-1]).any(axis=(1, 2))
    return (int((open_ & (status == M.TRUE)).sum()), int((open_ & alive & g_moved).sum()), int((open_ & alive & ~g_moved & ~ops_moved).sum()),
            int((~open_ & alive & ops_moved).sum()), int((~open_ & ~alive).sum()))


def interval_table_counts(name, form):
    _, _, L, U, open_ = interval_table(name, form)
    lb, ub, _, st = interval_table_reference(name, form)
    return table_counts(np.stack([L, U], axis=2), np.stack([lb, ub], axis=2), st, open_)


def set_table_counts(name, form, sw, base):
    _, _, bits, open_ = set_table(name, form, sw, base)
    ref = set_table_reference(name, form, sw, base)
    return table_counts(bits, ref[2], ref[4], open_)


# ------------------------------------------------------------------------------------------------------------- (b) random stores
def view_value(v, sol):
    if isinstance(v, M.Identity):
        return int(sol[v.idx])
    if isinstance(v, M.Addition):
        return view_value(v.x, sol) + v.v
    if isinstance(v, M.Constant):
        return v.value
    return sum(view_value(m, sol) for m in v.vars)


def holds(f, sol):
    """Truth of a formula under a full assignment."""
    if isinstance(f, (M.And, M.Conjunction)):
        return all(holds(g, sol) for g in f.fs)
    if isinstance(f, M.Or):
        return any(holds(g, sol) for g in f.fs)
    o = [view_value(v, sol) for v in f.ops]
    k = f.kind
    if k == M.NEQ:
        return o[0] != o[1]
    if k == M.EQ:
        return o[0] == o[1]
    if k == M.LT:
        return o[0] < o[1]
    if k == M.LT3:
        return o[0] < o[1] + o[2]
    if k == M.GT3:
        return o[0] > o[1] + o[2]
    if k == M.EQ3:
        return o[0] == o[1] + o[2]
    if k == M.MUL3:
        return o[0] == o[1] * o[2]
    return (o[0] == 1) == (k == M.BOOL)


def random_leaf_store(seed, n_vars, n_units, dom, set_mode=False, n_strong=10):
    """(vs, cs, sol): a store in the style of test_reified.random_formula_store whose leaves also draw XEqYPlusZ and, in interval mode,
    XEqYMulZ (factors from three extra variables over (0, 3), the x view shifted by -dom[0]) and XLessY against Sum((b, c)).  Ternary
    kinds carry an offset that centres y + z on the domain, so that their thresholds are met on negative domains too.  Every unit holds
    under the planted assignment `sol` (units are redrawn until they do), so a box around it never fails.  The first `n_strong` units are
    the nested mix (a quarter And; 15 % stand-alone x < y + c), the rest weak Ors of two or three leaves, as setform_cases.wide_case adds.
    The kinds are dealt from a shuffled deck, so a store of a dozen leaves has every kind."""
    rng = splitmix64(seed)
    vs, cs = M.VStore(), M.CStore()
    n_x = n_vars - 3 - (0 if set_mode else 3)
    xs = [vs.alloc(dom) for _ in range(n_x)]
    bs = [vs.alloc((0, 1)) for _ in range(3)]
    ms = [] if set_mode else [vs.alloc((0, 3)) for _ in range(3)]
    sol = np.concatenate([rng.integers(dom[0], dom[1] + 1, n_x), rng.integers(0, 2, 3), rng.integers(0, 4, len(ms))]).astype(np.int32)
    mid = (dom[0] + dom[1]) // 2
    all_kinds = ["NEQ", "EQ", "LT", "LT3", "GT3", "LTC", "EQ3"] + ([] if set_mode else ["MUL3", "LTSUM"])
    deck = []

    def deal(negatable):
        if not any(k not in ("EQ3", "MUL3") or not negatable for k in deck):
            deck.extend(all_kinds[i] for i in rng.permutation(len(all_kinds)))
        for i, k in enumerate(deck):
            if k not in ("EQ3", "MUL3") or not negatable:
                return deck.pop(i)

    def leaf(negatable=False):
        k = deal(negatable)
        a, b, c = (xs[i] for i in rng.choice(n_x, size=3, replace=False))
        off = int(rng.integers(-2, 3))
        if k == "NEQ":
            return M.XNeqY(a, M.Addition(b, off))
        if k == "EQ":
            return M.XEqY(a, M.Addition(b, off))
        if k == "LT":
            return M.XLessY(a, M.Addition(b, off))
        if k == "LT3":
            return M.XLessYPlusZ(a, b, M.Addition(c, off - mid))
        if k == "GT3":
            return M.XGreaterYPlusZ(a, b, M.Addition(c, off - mid))
        if k == "EQ3":
            return M.XEqYPlusZ(a, b, M.Addition(c, off - mid))
        if k == "MUL3":
            y, z = (ms[i] for i in rng.choice(3, size=2, replace=False))
            return M.XEqYMulZ(M.Addition(a, -dom[0]), y, z)
        if k == "LTSUM":
            return M.XLessY(M.Addition(a, mid + off), M.Sum((b, c)))
        return M.XLessY(a, M.Constant(int(rng.integers(dom[0], dom[1] + 1))))

    def boolean():
        b = bs[int(rng.integers(0, 3))]
        return M.Boolean(b) if rng.random() < 0.5 else M.BooleanNeg(b)

    def formula(depth, negatable=False):
        # (no Boolean as a Conjunction's child: Boolean::propagate on a variable already 0 is a non-monotonic update, the reference
        # panics — see random_formula_store; Booleans enter as Disjunction children)
        if depth == 0 or rng.random() < 0.3:
            return leaf(negatable)
        kids = tuple(formula(depth - 1, negatable) for _ in range(int(rng.integers(2, 4))))
        if rng.random() < 0.25:
            return M.And(kids)
        if rng.random() < 0.4:
            kids = kids + (boolean(),)
        return M.Or(kids)

    def strong():
        u = rng.random()
        if u < 0.15:
            a, b = (xs[i] for i in rng.choice(n_x, size=2, replace=False))
            return M.XLessY(a, M.Addition(b, int(rng.integers(-2, 3))))
        if u < 0.45:
            return M.implication(formula(1), leaf(True))
        if u < 0.65:
            return M.equivalence(M.Boolean(bs[int(rng.integers(0, 3))]), formula(1, True))
        f = formula(2)
        return f if M.is_formula_unit(f) else M.Or((f, leaf()))

    def weak():
        kids = [leaf() for _ in range(int(rng.integers(2, 4)))]
        if rng.random() < 0.3:
            kids[int(rng.integers(0, len(kids)))] = boolean()
        return M.Or(tuple(kids))

    for k in range(n_units):
        for _ in range(1000):
            u = strong() if k < n_strong else weak()
            if holds(u, sol):
                break
        else:
            raise AssertionError("no unit that the planted assignment satisfies")
        cs.alloc(u)
    return vs, cs, sol


N_NODES = 201
BATCHES = (1, 3, 5, 201)
TIGHT = (1.0, 0.9, 0.75, 0.5)
ACTIVE_KINDS = ("full", "off10", "off50", "last")


def mixed_boxes(seed, vs, sol, n_nodes=N_NODES):
    """Even nodes: random sub-boxes (a variable is narrowed with probability 0.25).  Odd nodes: boxes around the planted assignment,
    a variable assigned to it with probability 1, 0.9, 0.75, 0.5 in turn and else drawn around it."""
    rng = splitmix64(seed)
    lb0, ub0 = vs.bounds()
    L = np.tile(lb0, (n_nodes, 1)); U = np.tile(ub0, (n_nodes, 1))
    for k in range(n_nodes):
        tight = TIGHT[(k // 2) % 4]
        for v in range(len(lb0)):
            if k % 2 == 0:
                if rng.random() < 0.25:
                    a = int(rng.integers(lb0[v], ub0[v] + 1)); L[k, v], U[k, v] = a, int(rng.integers(a, ub0[v] + 1))
            elif rng.random() < tight:
                L[k, v] = U[k, v] = sol[v]
            else:
                L[k, v], U[k, v] = int(rng.integers(lb0[v], sol[v] + 1)), int(rng.integers(sol[v], ub0[v] + 1))
    return L.astype(np.int32), U.astype(np.int32)


def mixed_sets(seed, vs, sol, sw, base, n_nodes=N_NODES):
    """The set-valued twin of mixed_boxes: random subsets with holes; around the planted assignment, singletons and subsets that hold it."""
    rng = splitmix64(seed)
    lb0, ub0 = vs.bounds()
    bits = random_sets(seed + 1, lb0, ub0, n_nodes, sw, base, p_keep=0.8)
    around = random_sets(seed + 2, lb0, ub0, n_nodes, sw, base, sol=sol, p_keep=0.4)
    single = M.interval_bits(sol, sol, sw, base)
    for k in range(1, n_nodes, 2):
        assigned = rng.random(len(lb0)) < TIGHT[(k // 2) % 4]
        bits[k] = np.where(assigned[:, None], single, around[k])
    return bits


def active_rows(kind, n_nodes, n_units, seed):
    if kind == "full":
        return orc.full_active(n_nodes, n_units)
    if kind == "last":
        a = np.zeros((n_nodes, (n_units + 63) // 64), np.uint64)
        a[:, (n_units - 1) >> 6] = np.uint64(1) << np.uint64((n_units - 1) & 63)
        return a
    return random_active(seed, n_nodes, n_units, p_off=0.1 if kind == "off10" else 0.5)


# (name, seed, domain, units, variables): every domain at every unit count; the variable counts put the slots on both sides of 32 and 64
RANDOM_CASES = {
    "p6": (7101, (0, 6), 6, 12), "p34": (7102, (0, 6), 34, 40), "p66": (7103, (0, 6), 66, 70), "p130": (7104, (0, 6), 130, 40),
    "z6": (7111, (-4, 5), 6, 40), "z34": (7112, (-4, 5), 34, 12), "z66": (7113, (-4, 5), 66, 40), "z130": (7114, (-4, 5), 130, 70),
    "n6": (7128, (-9, -2), 6, 70), "n34": (7122, (-9, -2), 34, 40), "n66": (7123, (-9, -2), 66, 12), "n130": (7124, (-9, -2), 130, 70),
}
FOREST_CASES = ("p34", "z34", "n34")
# set mode: one word that starts just below the domain; the zero-crossing domain on two words with -1 | 0 at the word boundary
SET_RANDOM_LAYOUT = {(0, 6): (1, -1), (-4, 5): (2, -64), (-9, -2): (1, -10)}


@functools.lru_cache(maxsize=None)
def random_case(name):
    """(vs, cs, sol, L, U)."""
    seed, dom, n_units, n_vars = RANDOM_CASES[name]
    vs, cs, sol = random_leaf_store(seed, n_vars, n_units, dom)
    return (vs, cs) + frozen((sol,) + mixed_boxes(seed + 500, vs, sol))


@functools.lru_cache(maxsize=None)
def random_reference(name, kind="full"):
    """(lb, ub, active, status) of the oracle on random_case's nodes under the `active` rows of that kind."""
    vs, cs, _, L, U = random_case(name)
    act = active_rows(kind, L.shape[0], len(cs), RANDOM_CASES[name][0] + 900)
    return frozen(oracle_model(vs, cs).consistency(L, U, act)[:4])


@functools.lru_cache(maxsize=None)
def set_random_case(name):
    """(vs, cs, sol, bits, sw, base)."""
    seed, dom, n_units, n_vars = RANDOM_CASES[name]
    sw, base = SET_RANDOM_LAYOUT[dom]
    vs, cs, sol = random_leaf_store(seed + 50, n_vars, n_units, dom, set_mode=True)
    return (vs, cs) + frozen((sol, mixed_sets(seed + 550, vs, sol, sw, base))) + (sw, base)


@functools.lru_cache(maxsize=None)
def set_random_reference(name, kind="full"):
    """(lb, ub, bits, active, status)."""
    vs, cs, _, bits, sw, base = set_random_case(name)
    act = active_rows(kind, bits.shape[0], len(cs), RANDOM_CASES[name][0] + 950)
    return frozen(oracle_model(vs, cs).consistency_set(bits, base, act)[:5])


def leaf_kinds(cs, n_vars):
    """The kinds in the lowered leaf tables of every unit, and whether a Sum operand occurs — read from the lowering's output."""
    kinds, sums = set(), []
    for p in cs.pushes(n_vars, sums_out=sums):
        kinds |= {int(k) for k in p[-1]["kind"]}
    return kinds, len(sums) > 0


# ------------------------------------------------------------------------------------------------------------- (c) mask edges
N_EDGE = 96


@functools.lru_cache(maxsize=None)
def mask_edge_case():
    """(vs, cs, L, U).  Units: 0 an equivalence, 1 x0 < x1 + 1, 2 an Or of 63 leaves (a tree of exactly 64 nodes: its last leaf is bit 63),
    3 an And of an Or of 30 and an Or of 31 leaves (64 nodes again; the second Or's child mask is shifted by 33), 4 Distinct over 12
    variables (66 leaves: a flat Conjunction of 67 nodes, the member loop), 5 an implication.  Every leaf of the two wide units has a
    variable of its own in (-2, 3): y_i < 0, z_i != 1 or z_i = 2.  A node disentails most of them (a box inside 0..3, the singleton 1, a
    box without 2), leaves a few open — one, so that the unit propagates it; two; none, so that the node fails — or entails one; the open
    and entailed positions walk down from the last child.  Unit 3's other Or keeps one child open wherever the node is not meant to fail."""
    rng = splitmix64(6464)
    vs, cs = M.VStore(), M.CStore()
    xs = [vs.alloc((0, 13)) for _ in range(12)]
    b = vs.alloc((0, 1))
    ys = [vs.alloc((-2, 3)) for _ in range(63)]
    zs = [vs.alloc((-2, 3)) for _ in range(61)]
    zleaf = [M.XNeqY(z, M.Constant(1)) if i % 2 == 0 else M.XEqY(z, M.Constant(2)) for i, z in enumerate(zs)]
    cs.alloc(M.equivalence(M.Boolean(b), M.XLessY(xs[0], xs[1])))
    cs.alloc(M.x_leq_y(xs[0], xs[1]))
    cs.alloc(M.Or(tuple(M.XLessY(y, M.Constant(0)) for y in ys)))
    cs.alloc(M.And((M.Or(tuple(zleaf[:30])), M.Or(tuple(zleaf[30:])))))
    cs.alloc(M.Distinct(xs))
    cs.alloc(M.implication(M.XNeqY(xs[2], xs[3]), M.XLessY(xs[4], M.Constant(5))))
    assert [len(M.lower_formula(cs.units[u], len(vs))[0]) for u in (2, 3, 4)] == [64, 64, 67]
    lb0, ub0 = vs.bounds()
    L = np.tile(lb0, (N_EDGE, 1)); U = np.tile(ub0, (N_EDGE, 1))
    y0, z0 = 13, 13 + 63
    for k in range(N_EDGE):
        plant = np.sort(rng.permutation(14)[:12])[np.r_[0, 1, 2 + rng.permutation(10)]]  # distinct values with x0 < x1
        for v in range(12):  # the ordinary part: boxes around distinct values, many variables assigned (the Distinct removes their values)
            u = rng.random()
            if u < 0.5:
                L[k, v] = U[k, v] = plant[v]
            elif u < 0.8:
                L[k, v], U[k, v] = int(rng.integers(0, plant[v] + 1)), int(rng.integers(plant[v], 14))
        mode = k % 4  # 0: one child open, 1: two open, 2: none open (the node fails), 3: one child entailed
        for i in range(63):
            a = int(rng.integers(0, 4)); L[k, y0 + i], U[k, y0 + i] = a, int(rng.integers(a, 4))        # y_i < 0 disentailed
        for i in range(61):
            if i % 2 == 0:
                L[k, z0 + i] = U[k, z0 + i] = 1                                                           # z_i != 1 disentailed
            else:
                L[k, z0 + i], U[k, z0 + i] = (-2, int(rng.integers(-2, 2))) if rng.random() < 0.5 else (3, 3)  # z_i = 2 disentailed
        py = (62 - k // 4) % 63 if k % 8 < 4 else int(rng.integers(0, 63))   # the last child first, then down to the first
        pz = (60 - k // 4) % 61 if k % 8 < 4 else int(rng.integers(0, 61))
        q = pz + 30 if pz < 30 else (pz - 30) % 30  # a child of unit 3's other Or: open, so that both halves hold
        def open_(v):  # (z_i != 1 on (1, 3): the bound 1 goes, in interval mode too)
            L[k, v], U[k, v] = (1, 3) if v >= z0 and (v - z0) % 2 == 0 else (-2, 3)
        if mode in (0, 1):
            for p, n, base in ((py, 63, y0), (pz, 61, z0)):
                open_(base + p)
                if mode == 1:
                    open_(base + (p + 17) % n)
            open_(z0 + q)
        elif mode == 3:
            L[k, y0 + py], U[k, y0 + py] = -2, -1
            L[k, z0 + pz], U[k, z0 + pz] = (0, 0) if pz % 2 == 0 else (2, 2)
            open_(z0 + q)
    return (vs, cs) + frozen((L.astype(np.int32), U.astype(np.int32)))


MASK_SET_LAYOUT = (1, -2)


@functools.lru_cache(maxsize=None)
def mask_edge_reference(set_mode=False):
    vs, cs, L, U = mask_edge_case()
    om = oracle_model(vs, cs)
    if set_mode:
        sw, base = MASK_SET_LAYOUT
        return frozen(om.consistency_set(M.interval_bits(L, U, sw, base), base, None)[:5])
    return frozen(om.consistency(L, U, None)[:4])


def not_flat_65():
    """(vs, cs): one unit of 65 tree nodes that is not a flat Conjunction — And((Or of 63 leaves,)) — next to a plain unit."""
    vs, cs = M.VStore(), M.CStore()
    ys = [vs.alloc((-2, 3)) for _ in range(63)]
    cs.alloc(M.XLessY(ys[0], ys[1]))
    cs.alloc(M.And((M.Or(tuple(M.XLessY(y, M.Constant(0)) for y in ys)),)))
    assert len(M.lower_formula(cs.units[1], len(vs))[0]) == 65
    return vs, cs
