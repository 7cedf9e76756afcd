"""Set mode beyond two words and past the changed-variable list — TEST INFRASTRUCTURE shared by test_set_wide_cpu.py and test_set_wide_gpu.py:
the generators of the cases and their references (OracleModel.consistency_set / search_set and the host judges of enum_set_ref.py /
test_bnb_host.py).  A generator is a pure function of its arguments (fixed seeds); a reference is computed once, cached here, shared by the
tests and never changed.  What is a property of the inputs or of the reference alone is asserted in test_set_wide_cpu.py, without a GPU.

Values and bit positions: value v of a set is bit v - base; "position p" below always means the bit, base + p the value."""
import functools

import numpy as np

from oracle import oracle as orc
from pcp_amd import model as M

from enum_set_ref import SET_KINDS, reference_dfs
from test_set_mode import random_sets
from util import random_active, random_csp, splitmix64


def bits_of_positions(rows, sw):
    """[len(rows), sw] uint64 from rows[i] = the bit positions of entry i."""
    out = np.zeros((len(rows), sw), np.uint64)
    for i, ps in enumerate(rows):
        for p in ps:
            p = int(p)
            assert 0 <= p < 64 * sw
            out[i, p >> 6] |= np.uint64(1) << np.uint64(p & 63)
    return out


def cardinality(bits):
    """Number of members of every set of bits[..., sw]."""
    return np.unpackbits(np.ascontiguousarray(bits, np.uint64).view(np.uint8), axis=-1).sum(axis=-1)


# ------------------------------------------------------------------------------------------- 1. fixpoints at 3, 5 and 8 words
# (set_words, base, hi): the first three fill the universe exactly (hi - base + 1 == 64 * set_words); the last one ends inside its last
# word, so the top bits of every set are clear and a shift must not bring anything in from there.
SHAPES = [(3, -70, 121), (5, -70, 249), (8, -200, 311), (8, -200, 290)]
DENSITIES = {"planted400": (400, True), "planted70": (70, True), "unplanted70": (70, False)}
FIX_VARS = (90, 91)  # V * set_words even and odd at 3 and 5 words: the 16-byte and the scalar staging path, every second row misaligned
FIX_NODES = 32
FIX_SEEDS = (0, 1, 2)


def fixpoint_case(sw, base, hi, V, density, seed):
    """(props, bits [32, V, sw], active [32, words]): a random CSP over all six set-mode kinds on [base, hi], random subsets with holes."""
    P, planted = DENSITIES[density]
    s = seed + 10 * V + 1000 * sw + 100000 * list(DENSITIES).index(density) + (7 if hi == 290 else 0)
    props, lb, ub, sol = random_csp(41000 + s, V, P, planted=planted, dom=(base, hi), kinds=SET_KINDS)
    bits = random_sets(42000 + s, lb, ub, FIX_NODES, sw, base, sol if planted else None)
    act = random_active(43000 + s, FIX_NODES, P, p_off=0.1)
    return props, bits, act


# ------------------------------------------------------------------------------------------- 2. shifts at word edges, aimed
SHIFT_BASE = -70
SHIFT_KINDS = ("eq", "neq", "lt", "eq_const", "neq_const")


def shift_offsets(sw):
    """0, +-1, +-63, +-64, +-65, +-127, +-128 and the three magnitudes around the universe's size (the last two shift everything out)."""
    n = 64 * sw
    return [0] + [s * m for m in (1, 63, 64, 65, 127, 128, n - 1, n, n + 5) for s in (1, -1)]


def edge_positions(sw):
    return [0, 63, 64, 127, 128, 64 * sw - 1]


def shift_constants(sw):
    """The values c of `x ◇ Constant(c) + d`: the first bit, bit 0 of the second word, the last bit."""
    return [SHIFT_BASE, SHIFT_BASE + 64, SHIFT_BASE + 64 * sw - 1]


def shift_model(kind, d, c=None):
    """(n_vars, props): x ◇ y + d over two variables, or x ◇ Constant(c) + d over one."""
    y = M.Identity(1) if c is None else M.Constant(int(c))
    unit = {"eq": M.XEqY, "neq": M.XNeqY, "lt": M.XLessY}[kind.split("_")[0]](M.Identity(0), M.Addition(y, int(d)))
    V = 2 if c is None else 1
    return V, M.lower_units([unit], V)


def shift_nodes(kind, sw, d, c=None):
    """bits [n, V, sw]: one node per pair of sets.  Every set holds members on the edge positions 0, 63, 64, 127, 128, 64 sw - 1 or is a
    singleton on one of them; the other side then contains or lacks the value the singleton hits through the offset."""
    n = 64 * sw
    E = edge_positions(sw)
    rng = splitmix64(5000 + 7 * sw + 1000 * SHIFT_KINDS.index(kind) + (d % 1009) + (0 if c is None else int(c) % 97))
    rnd = lambda k: [int(p) for p in rng.choice(n, size=k, replace=False)]
    inside = lambda p: 0 <= p < n
    if c is not None:
        t = int(c) + d - SHIFT_BASE  # the position the constant operand names (possibly outside the universe)
        rows = [[E + rnd(6)], [E + rnd(40)], [list(range(n))], [[p for p in E + rnd(6) if p != t]], [[E[1], E[4]]]]
        rows += [[[p]] for p in E]
        if inside(t):
            rows += [[[t]], [E + rnd(6) + [t]], [[t, (t + 64) % n]]]
        return np.stack([bits_of_positions(r, sw) for r in rows])
    rows = [[E + rnd(6), E + rnd(6)], [E + rnd(6), E + rnd(6)], [E + rnd(40), E + rnd(40)],
            [list(range(n)), E + rnd(3)], [E + rnd(3), list(range(n))], [list(range(n)), list(range(n))], [rnd(8), rnd(8)]]
    for p in E:
        # x = {p}: x = y + d names position p - d of y.  y = {p}: position p + d of x.
        for single_is_x, hit in ((True, p - d), (False, p + d)):
            holds = E + rnd(5) + ([hit] if inside(hit) else [])
            lacks = [q for q in E + rnd(6) if q != hit]
            for other in (holds, lacks) + (([hit],) if inside(hit) else ()):
                rows.append([[p], other] if single_is_x else [other, [p]])
    return np.stack([bits_of_positions(r, sw) for r in rows])


@functools.lru_cache(maxsize=None)
def shift_reference(kind, sw, d, c=None):
    """(bits_in, reference) of one model's batch; the reference = consistency_set(...)[:5] with every unit active."""
    V, props = shift_model(kind, d, c)
    bits = shift_nodes(kind, sw, d, c)
    return bits, orc.OracleModel(V, props).consistency_set(bits, SHIFT_BASE)[:5]


# ------------------------------------------------------------------------------------------- 3. more changed variables than the list holds
CAP = 64           # the list capacity the tests set ("list_cap"); the kernels' C = min(list_cap, 1024)
OVF_SW, OVF_BASE = 3, -70
ROOT_BASE = -3      # the forest roots built from these constructions: every position is >= 3, so every value is >= 0 (see forest_case)
OVF_NODES = 16
LEAVES = 100
# (a, b1, b2, c) as positions: the hub's value and the leaves' other values, in different words and on word edges
STAR_VARIANTS = [(64, 0, 191, 130), (191, 63, 128, 5), (0, 127, 64, 190)]


def _neq_rows(pairs):
    """pcp_prop rows of x != y + d for (x, y, d) in pairs, one unit each."""
    p = np.zeros(len(pairs), dtype=M.PROP_DTYPE)
    p["var"][:] = M.PCP_NOVAR
    p["kind"] = M.NEQ
    p["group"] = np.arange(len(pairs))
    for r, (x, y, d) in enumerate(pairs):
        p[r]["var"][0], p[r]["var"][1], p[r]["off"][1] = x, y, d
    return p


def _star_pairs():
    """Hub 0, leaves 1..100: x0 != x_i, then the ring x_i != x_{i+1} closed from leaf 100 to leaf 1."""
    return [(0, i, 0) for i in range(1, LEAVES + 1)] + [(i, i % LEAVES + 1, 0) for i in range(1, LEAVES + 1)]


@functools.lru_cache(maxsize=None)
def neq_star(variant):
    """All-XNeqY star with a ring among the leaves, implicit nodes.  Returns (V, props, bits [16, 101, 3], two_valued [16]).
    Why round 0 overflows: the hub {a} is the only singleton of the input (every leaf has two values or more), so the sweep runs the hub's
    100 records and takes `a` out of every leaf that holds it.  70 leaves per node are {a, b}: they become singletons.  On an all-XNeqY
    model only singletons are listed, so round 0 lists at least those 70 > 64 variables and takes the sweep over every record; there the
    ring records between two such leaves see both ends changed (the dedup picks the lower), and a leaf left with {b1, b2} loses the value
    of its neighbour.  Even nodes give leaf i the value b_(i mod 2), so ring neighbours differ and the node lives; odd nodes draw b at
    random and two equal neighbours fail them.  two_valued = the number of {a, b} leaves per node (asserted > 64 on the CPU)."""
    a, b1, b2, c = STAR_VARIANTS[variant]
    rng = splitmix64(6100 + variant)
    V = LEAVES + 1
    bits = np.zeros((OVF_NODES, V, OVF_SW), np.uint64)
    two_valued = np.zeros(OVF_NODES, np.int64)
    for k in range(OVF_NODES):
        rows = [[a]]
        two = set(int(i) for i in rng.choice(LEAVES, size=70, replace=False))
        for i in range(LEAVES):
            b = (b1, b2)[(i + 1) % 2] if k % 2 == 0 else (b1, b2)[int(rng.integers(0, 2))]
            if i in two:
                rows.append([a, b])
            else:
                rows.append([[a, b1, b2], [b1, b2], [b1, b2, c]][int(rng.integers(0, 3))])  # (the last two already lack a)
        two_valued[k] = len(two)
        bits[k] = bits_of_positions(rows, OVF_SW)
    return V, _neq_rows(_star_pairs()), bits, two_valued


def neq_star_root(variant):
    """The star as ONE forest root: every leaf {a, b_(i mod 2)} but five, which keep three values after the root's fixpoint and are tied by a
    few more XNeqY records, so that a small tree is left below a root whose round 0 lists 95 > 64 singletons.  Returns (V, props, bits [1, V, 3])."""
    a, b1, b2, c = STAR_VARIANTS[variant]
    c2 = (c + 17) % (64 * OVF_SW)
    assert len({a, b1, b2, c, c2}) == 5
    opened = (10, 30, 50, 70, 90)
    rows = [[a]] + [[a, (b1, b2)[(i + 1) % 2]] + ([c, c2] if i + 1 in opened else []) for i in range(LEAVES)]
    pairs = _star_pairs() + [(10, 30, 0), (10, 50, 0), (30, 50, 0), (70, 90, 0)]
    return LEAVES + 1, _neq_rows(pairs), bits_of_positions(rows, OVF_SW)[None]


@functools.lru_cache(maxsize=None)
def assigned_fallback(variant, n_single=70, n_open=30, n_nodes=OVF_NODES, root=False):
    """All-XNeqY, implicit nodes whose INPUT holds n_single > 64 singletons: the sweep cannot list the assigned variables and streams the
    table instead.  x != y + d with offsets up to two words, satisfied by a hidden solution; a singleton is its variable's hidden value, an
    open set holds the hidden value, values that assigned neighbours forbid and random ones.  Odd nodes move three singletons to random
    values (some of them fail).  Returns (V, props, bits [n_nodes, V, 3], singles [n_nodes] = the singletons of each input node).
    root=True (a forest root, one node): the open variables are the last n_open, each with the four values around its hidden one, and every
    pair of them has a record that forbids one combination of those — the records among open variables are not entailed at the root, so a
    tree is left below it."""
    rng = splitmix64(6200 + variant + 10 * n_open)
    V, n = n_single + n_open, 64 * OVF_SW
    sol = rng.integers(4, n - 2, size=V)  # positions
    pairs = []
    for _ in range(4 * V):
        x, y = (int(v) for v in rng.choice(V, size=2, replace=False))
        d = int(rng.integers(-140, 141))
        if sol[x] == sol[y] + d:
            d += 1
        pairs.append((x, y, d))
    if root:
        pairs += [(x, y, int(sol[x] - sol[y]) + 1) for x in range(n_single, V) for y in range(x + 1, V)]
    incident = [[] for _ in range(V)]  # variable -> (the other variable, s): an assigned other forbids its value + s here
    for x, y, d in pairs:
        incident[x].append((y, d))
        incident[y].append((x, -d))
    bits = np.zeros((n_nodes, V, OVF_SW), np.uint64)
    for k in range(n_nodes):
        single = np.zeros(V, bool)
        single[np.arange(n_single) if root else rng.choice(V, size=n_single, replace=False)] = True
        val = sol.copy()
        if k % 2:
            moved = rng.choice(np.nonzero(single)[0], size=3, replace=False)
            val[moved] = rng.integers(0, n, size=3)
        rows = []
        for v in range(V):
            if single[v]:
                rows.append([val[v]])
                continue
            forbidden = [int(val[o] + s) for o, s in incident[v] if single[o]]
            forbidden = [p for p in forbidden if 3 <= p < n and p != sol[v]]
            more = [sol[v] - 1, sol[v] + 1, sol[v] + 2] if root else [int(p) for p in rng.choice(n, size=int(rng.integers(1, 4)), replace=False)]
            rows.append([sol[v]] + forbidden[:3] + more)
        bits[k] = bits_of_positions(rows, OVF_SW)
    return V, _neq_rows(pairs), bits, (cardinality(bits) == 1).sum(axis=1)


@functools.lru_cache(maxsize=None)
def mixed_star(variant, n_nodes=OVF_NODES, root=False):
    """The star and ring of neq_star plus XLessY records and one ternary record, so the model is not all-XNeqY: every changed variable is
    listed, a singleton or not.  Hub 0 = {a}, leaves 1..100 three-valued, variable 101 wide.  Returns (V, props, bits [n_nodes, 102, 3],
    holders [n_nodes, 100] bool = which leaves hold `a` in the input).
    Why round 0 overflows: the sweep runs every live record once; the hub's record of a leaf that holds `a` takes it out and marks the leaf,
    so round 0 lists at least as many variables as there are such leaves with a live hub record — 85 per node as generated, and with the
    `active` rows of the tests still more than 64 (both counted on the CPU).
    root=True: ONE node for the forest.  The XLessY records are x_i < x_0 for all leaves but four, every b_i lies below a and every c_i above:
    those 96 leaves end as {b_i} (ring neighbours differ); the four others keep b_i, c_i and two more values above a, are chained by
    x_i < x_j + 100 (neither entailed nor failing at the root) and two of them meet variable 101 in the ternary record."""
    a = (100, 70, 126)[variant]  # inside the second word, at its ends in the other variants
    rng = splitmix64(6300 + variant + (50 if root else 0))
    n, V = 64 * OVF_SW, LEAVES + 2
    opened = (10, 30, 50, 70)
    units = [M.XNeqY(M.Identity(x), M.Addition(M.Identity(y), d)) for x, y, d in _star_pairs()]
    if root:
        units += [M.XLessY(M.Identity(i), M.Identity(0)) for i in range(1, LEAVES + 1) if i not in opened]
        units += [M.XLessY(M.Identity(i), M.Addition(M.Identity(j), 100)) for i, j in zip(opened, opened[1:])]
    else:
        for _ in range(12):
            i, j = (int(v) for v in rng.choice(np.arange(1, LEAVES + 1), size=2, replace=False))
            units.append(M.XLessY(M.Identity(i), M.Addition(M.Identity(j), int(rng.integers(40, 161)))))
    # in positions: p101 = p10 + p30 - 90, at the root p101 < p10 + p30 - 90
    units.append((M.XLessYPlusZ if root else M.XEqYPlusZ)(M.Identity(V - 1), M.Identity(10), M.Addition(M.Identity(30), -(ROOT_BASE if root else OVF_BASE) - 90)))
    props = M.lower_units(units, V)
    bits = np.zeros((n_nodes, V, OVF_SW), np.uint64)
    holders = np.zeros((n_nodes, LEAVES), bool)
    for k in range(n_nodes):
        rows = [[a]]
        lack = set() if root else set(int(i) for i in rng.choice(LEAVES, size=15, replace=False))
        prev_b = first_b = -1
        for i in range(LEAVES):
            while True:
                b = int(rng.integers(3, a)) if root else int(rng.integers(0, n))
                if b != a and b != prev_b and not (i == LEAVES - 1 and b == first_b):  # (the ring is closed: leaf 100 meets leaf 1)
                    break
            prev_b = b
            first_b = b if i == 0 else first_b
            c = int(rng.integers(a + 1, n))
            e = int(rng.integers(0, n))
            if not root:  # three distinct values, none of them a
                b, c, e = (int(p) for p in rng.choice(np.delete(np.arange(n), a), size=3, replace=False))
            rows.append([b, c, e] if i in lack else [a, b, c])
            if root and i + 1 in opened:
                rows[-1] += [int(p) for p in rng.integers(a + 1, n, size=2)]
            holders[k, i] = i not in lack
        rows.append(list(range(0, n, 3)) if not root else [40, 60, 80, 100, 120, 140, 160])
        bits[k] = bits_of_positions(rows, OVF_SW)
    return V, props, bits, holders


def mixed_star_active(variant, n_units):
    """The `active` rows of the mixed star's explicit run: about one unit in ten switched off."""
    return random_active(6400 + variant, OVF_NODES, n_units, p_off=0.1)


@functools.lru_cache(maxsize=None)
def overflow_roots():
    """name -> (V, props, root [1, V, 3]) over ROOT_BASE: the three constructions as forest roots (total > C on an all-XNeqY and on a mixed
    model, ns > C), each with a small tree below it."""
    return {"neq_star": neq_star_root(1), "assigned": assigned_fallback(1, 70, 5, 1, True)[:3], "mixed_star": mixed_star(1, 1, True)[:3]}


def overflow_random_csp():
    """Item 1's planted P = 400 shape at three words (V = 91, so the scalar row path as well), for list_cap = 64."""
    sw, base, hi = SHAPES[0]
    return (91, sw, base, hi) + fixpoint_case(sw, base, hi, 91, "planted400", 3)


# ------------------------------------------------------------------------------------------- 4. the forest kernel on wide sets
FOREST_SW = (3, 5)
FOREST_BRANCHERS = [("split", "middle"), ("enumerate", "middle"), ("enumerate", "min")]
FOREST_SEEDS = {  # chosen on the CPU so that every reference tree has 30 .. 5000 nodes (test_set_wide_cpu.py asserts it)
    ("split", 3): (3, 5), ("split", 5): (9, 15), ("enumerate", 3): (15, 21), ("enumerate", 5): (1, 26),
}
FOREST_STEPS = (3, 64)


def forest_case(sw, brancher, seed):
    """(V, props, root [1, V, sw], base, hull): 6..10 variables of 3..6 members drawn over the whole universe, a planted CSP over all six kinds
    on those values (offsets span words).  Under BinarySplit every value is >= 0 over a negative base — the reference's MiddleVal truncates
    toward zero and {-3, -2} branches to itself —, under Enumerate values are negative too."""
    base = -3 if brancher == "split" else -70
    lo, hi = (0 if brancher == "split" else base), base + 64 * sw - 1
    s = 7000 + 100 * sw + 10 * (brancher == "split") + seed
    rng = splitmix64(s)
    V = int(rng.integers(6, 11))
    third = (hi - lo) // 3
    props, _, _, sol = random_csp(s + 500, V, int(rng.integers(V, 2 * V)), planted=True, dom=(lo + third, hi - third), kinds=SET_KINDS)
    # the members: the hidden value moved by shifts from one pool of eight shared by the variables, up to a third of the universe either way
    # — x = y + c then holds for every shift both sides share, so the root's fixpoint leaves a tree (random members would all be pruned)
    pool = [0] + [int(x) for x in rng.integers(-third, third + 1, size=7)]
    rows = []
    for v in range(V):
        k = int(rng.integers(3, 7))
        members = {int(sol[v]) - base}
        while len(members) < k:
            members.add(int(sol[v]) + pool[int(rng.integers(0, 8))] - base)
        rows.append(sorted(members))
    return V, props, bits_of_positions(rows, sw)[None], base, (base, hi)


@functools.lru_cache(maxsize=None)
def forest_reference(sw, brancher, val, seed, first_only=False):
    V, props, root, base, _ = forest_case(sw, brancher, seed)
    return tree_reference(("wide", sw, brancher, seed), V, props, root, base, brancher, val, first_only)


def tree_reference(key, V, props, root, base, brancher, val, first_only=False):
    """dict(nodes, solutions, failed, first): OracleModel.search_set below `root` under BinarySplit, the judge of enum_set_ref.py under Enumerate."""
    if brancher == "enumerate":
        r = reference_dfs(key, V, props, root[0], base, val, first_only=first_only)
        return {k: r[k] for k in ("nodes", "solutions", "failed", "first")}
    ss, _, _, first = orc.OracleModel(V, props).search_set(None, None, root.shape[2], base, all_solutions=not first_only, root_bits=root[0])
    return {"nodes": ss["num_nodes"], "solutions": ss["num_solution"], "failed": ss["num_failed_node"], "first": first if ss["num_solution"] else None}


BNB_SEEDS = {"split": 3, "enumerate": 3}  # (reference trees of 31 and 35 nodes)


def bnb_case(brancher, seed=None):
    """Branch and bound at three words: (V, props, lb0, ub0, var, mode, base).  Seven values around a hidden solution per variable, all >= 0
    over base -3; the objective is variable 0."""
    sw, base = 3, -3
    s = 7700 + 10 * (BNB_SEEDS[brancher] if seed is None else seed) + (brancher == "split")
    V = 8
    props, _, _, sol = random_csp(s, V, 6, planted=True, dom=(0, base + 64 * sw - 1), kinds=SET_KINDS)
    lb0 = np.maximum(sol - 3, 0).astype(np.int32)
    ub0 = np.minimum(sol + 3, base + 64 * sw - 1).astype(np.int32)
    return V, props, lb0, ub0, 0, ("min" if brancher == "split" else "max"), base


@functools.lru_cache(maxsize=None)
def bnb_reference(brancher):
    """The host specification the BnB forest tests use: reference_bnb_set under BinarySplit, reference_bnb_set_any under Enumerate (MiddleVal)."""
    from test_bnb_forest_cpu import reference_bnb_set_any
    from test_bnb_host import reference_bnb_set
    V, props, lb0, ub0, var, mode, base = bnb_case(brancher)
    om = orc.OracleModel(V, props)
    if brancher == "split":
        return reference_bnb_set(om, lb0, ub0, var, mode == "min", 3, base)
    return reference_bnb_set_any(om, lb0, ub0, var, mode == "min", 3, base, "enumerate", "middle")


# ------------------------------------------------------------------------------------------- 5. BinarySplit branching on wide sets
BRANCH_BASE = -3
BRANCH_WHERE = ("first", "middle", "last")


def branch_case(sw, where):
    """(bits [24, 40, sw], status [24], active [24, 1]) of a propagated-looking batch: sparse random sets of values >= 0, Unknown, True and False
    nodes mixed.  In every node the first variable of minimal cardinality > 1 has its two or three members in the first, a middle or the
    last word; every other variable is a singleton or has four members or more."""
    n_nodes, V, n = 24, 40, 64 * sw
    word = {"first": 0, "middle": sw // 2, "last": sw - 1}[where]
    rng = splitmix64(8000 + 10 * sw + BRANCH_WHERE.index(where))
    lo = -BRANCH_BASE  # position of value 0
    rows_all = []
    for _ in range(n_nodes):
        rows = []
        for v in range(V):
            k = 1 if rng.random() < 0.3 else int(rng.integers(4, 8))
            rows.append([int(p) for p in rng.choice(np.arange(lo, n), size=k, replace=False)])
        first = int(rng.integers(0, V - 1))
        w_lo = max(64 * word, lo)
        for j in (first, int(rng.integers(first + 1, V))):  # a tie: the lower index is taken
            rows[j] = [int(p) for p in rng.choice(np.arange(w_lo, 64 * word + 64), size=2 + (where == "middle"), replace=False)]
        rows_all.append(bits_of_positions(rows, sw))
    status = np.array([M.UNKNOWN, M.TRUE, M.FALSE] * (n_nodes // 3), np.uint8)
    rng.shuffle(status)
    active = rng.integers(0, 1 << 62, size=(n_nodes, 1)).astype(np.uint64)
    return np.stack(rows_all), status, active
