"""Shared cases of the small-store parity tests (test_small_cases_cpu.py, test_small_edges_gpu.py): inputs that put smallfix_kernel
(pcp_small.hip, one wavefront per node, plan.path 4) on the edges the random stores of test_gpu_parity.py do not reach.

A. The 128-value mask of the grouped all-different step: hulls of 126 .. 129 values from bases below and above zero, runs of taken
   values across the bits 31|32, 63|64 and 95|96 with a bound on the run, duplicates at bits 0, 64 and 127 (A1); a hull that starts
   beyond the mask and shrinks under it during the fixpoint (A2); units of 3, 63 and 64 variables (A3); nine Distinct units behind
   31 or 63 ordinary ones, under `active` rows that switch the first, the eighth and the ninth off (A4).
B. Staging: stores of exactly 63, 64, 65, 127 and 128 slots, stores of exactly 1 .. 129 units, `active` rows with the last unit off
   or alone; and the two stores just beyond the path's limits (129 slots, 2049 records).
C. The node loop: 12288 rows of the 64-variable store, rows of period 127 whose neighbours differ in status.
D. Node units on a store with a grouped Distinct, 0 .. 70 of them per node.

A case is (name, n_vars, props, L, U, active or None, expect); `expect` maps a description to a predicate over the oracle's
(lb, ub, active, status) that says the case reaches the edge it is named for — test_small_cases_cpu.py checks them all, so that
the GPU test cannot pass on inputs that miss.  Everything is seeded and computed once per process; the arrays are read-only."""
import functools

import numpy as np

from oracle import oracle as orc
from pcp_amd import model as M

from util import random_active, random_nodes, splitmix64


def frozen(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def oracle_rows(n_vars, props, L, U, act):
    """(lb, ub, active, status) of the oracle.  A row with lb > ub on input is a failed node for the device entries; the oracle, like the
    reference, cannot even allocate it (variable/store.rs:136): it gets the row with that domain mended, and the status is set."""
    bad = L > U
    ref = orc.OracleModel(n_vars, props).consistency(L, np.where(bad, L, U), act)[:4]
    ref[3][bad.any(axis=1)] = M.FALSE
    return frozen(ref)


@functools.lru_cache(maxsize=None)
def _reference(key):
    _, n_vars, props, L, U, act, _ = CASES[key]()
    return oracle_rows(n_vars, props, L, U, act)


def reference(key):
    """(lb, ub, active, status) of the oracle on the case CASES[key], under the case's own `active` rows (None: every unit)."""
    return _reference(key)


@functools.lru_cache(maxsize=None)
def implicit_reference(key):
    _, n_vars, props, L, U, act, _ = CASES[key]()
    return reference(key) if act is None else oracle_rows(n_vars, props, L, U, None)


# ---------------------------------------------------------------------------------------- what the lowering makes of a table
def unit_of_prop(props):
    """The unit of every row: a run of rows with one group_kind != 0 and one group is ONE unit (pcp_model_push_props)."""
    out, n = np.zeros(len(props), np.int64), -1
    for i in range(len(props)):
        same = i > 0 and props[i]["group_kind"] != 0 and props[i - 1]["group_kind"] == props[i]["group_kind"] and props[i - 1]["group"] == props[i]["group"]
        n += 0 if same else 1
        out[i] = n
    return out


def slot_count(props, n_vars):
    """n_slots of the lowered model (lower_model, pcp_lower.hip): the variables, then one slot per distinct Constant value."""
    consts = set()
    for p in props:
        arity = 1 if p["kind"] >= M.BOOL else (2 if p["kind"] <= M.LT else 3)
        consts |= {int(p["off"][i]) for i in range(arity) if p["var"][i] == M.PCP_CONST}
    return n_vars + len(consts)


# the limits of lower_alldiff (pcp_lower.hip, the line that sets `ok = n <= 64 && tab[0] < 8u && vars.size() + n <= 256 ...`) and of the tables
# pcp_small.hip keeps in LDS (kSmallAdUnits, kSmallAdVars): a change there has to be made here too
AD_MAX_VARS_PER_UNIT, AD_MAX_UNITS, AD_MAX_VARS = 64, 8, 256


def alldiff_units(props, n_vars):
    """(grouped, left): [(unit, its variables in lane order)] of the units lower_alldiff (pcp_lower.hip) enters into Lowered.ad_tab —
    a group of at least three rows, every one x != y without offset over variables, every pair of at most 64 variables exactly once,
    at most 8 units over at most 256 variables — and of the units that qualify but find the table full: those run pair by pair."""
    uop = unit_of_prop(props)
    grouped, left, n_tab_vars, r, P = [], [], 0, 0, len(props)
    while r < P:
        e = r
        while e < P and uop[e] == uop[r]:
            e += 1
        rows = props[r:e]
        if e - r >= 3 and rows[0]["group_kind"] != 0:
            x, y = rows["var"][:, 0].astype(np.int64), rows["var"][:, 1].astype(np.int64)
            ok = bool(((rows["kind"] == M.NEQ) & (rows["off"][:, 1] == rows["off"][:, 0]) & (x < n_vars) & (y < n_vars) & (x != y)).all())
            if ok:
                vs = sorted(set(x.tolist()) | set(y.tolist()))
                pairs = {(min(a, b), max(a, b)) for a, b in zip(x.tolist(), y.tolist())}
                n = len(vs)
                if n <= AD_MAX_VARS_PER_UNIT and len(pairs) == e - r == n * (n - 1) // 2:
                    if len(grouped) < AD_MAX_UNITS and n_tab_vars + n <= AD_MAX_VARS:
                        grouped.append((int(uop[r]), vs))
                        n_tab_vars += n
                    else:
                        left.append((int(uop[r]), vs))
        r = e
    return grouped, left


def hull(L, U, vs):
    """hi - lo of the variables `vs`, per row."""
    return U[:, vs].max(axis=1).astype(np.int64) - L[:, vs].min(axis=1)


def _statuses(*want):
    return lambda ref: all((ref[3] == s).any() for s in want)


ALL_STATUSES = _statuses(M.FALSE, M.TRUE, M.UNKNOWN)


# ---------------------------------------------------------------------------------------------------------------- A1 mask edges
A1_HULLS, A1_LOS, A1_M, A1_PER = (126, 127, 128, 129), (-130, -64, -1, 0, 5), 24, 14
A1_OFFS = (0, 31, 32, 63, 64, 95, 96, 127)
A1_WORDS = (32, 64, 96)  # the first bit of the mask's second, third and fourth word


def _a1_row(rng, H, lo, kind, turn=0):
    """One node over 24 variables, all in the unit.  Variable 0 holds the hull's lower end (assigned: the mask's base stays put),
    variable 1 its upper end; 2 .. 7 take a run, 8 and 9 carry the bounds set on it, 10 .. 19 the single offsets; 20 .. 23 are the
    operands of the XLessY records and stay wide except in the nodes built to end True.  `kind`: 0 .. 5 a bound on a run across a word
    boundary, 6 a duplicate, 7 an interval inside a run, 8 a node that ends True, 9 a hull that shrinks, 10 a mix."""
    m = A1_M
    l, u = np.full(m, lo, np.int64), np.full(m, lo + H, np.int64)
    l[0] = u[0] = lo
    l[1] = lo + H - 2
    taken = {0}

    def run(b):
        r = int(rng.integers(2, 7))
        s = int(rng.integers(b - r + 1, b))  # the run s .. s + r - 1 holds b - 1 and b
        for i in range(r):
            l[2 + i] = u[2 + i] = lo + s + i
        taken.update(range(s, s + r))
        return s, r

    def singles(p=0.5):
        nxt = 10
        for off in A1_OFFS:
            if off <= H - 3 and off not in taken and rng.random() < p:
                l[nxt] = u[nxt] = lo + off
                taken.add(off)
                nxt += 1

    if kind < 6:  # a bound on a run across one of the three word boundaries: the lower bound walks up over it, or the upper bound down
        s, r = run(A1_WORDS[kind % 3])
        a, b = (8, 9) if kind < 3 else (9, 8)
        l[a], u[a] = lo + s + int(rng.integers(0, 2)) * (A1_WORDS[kind % 3] - 1 - s), lo + H - 4   # on the run's first value, or on bit b - 1
        l[b], u[b] = lo + 2, lo + s + r - 1 - int(rng.integers(0, 2)) * (s + r - 1 - A1_WORDS[kind % 3])  # on its last value, or on bit b
        singles()
    elif kind == 6:  # two variables with one value, at bit 0, 64 or the hull's last bit (127 at most), in turn: a hull of 127 starts with bit 127
        d = (min(127, H), 0, 64)[turn % 3]
        run(A1_WORDS[int(rng.integers(0, 3))])
        l[10] = u[10] = l[11] = u[11] = lo + d
        if d == H:
            l[1] = lo + H
        if d == 0:
            l[11], u[11] = lo + H - 9, lo + H - 9
    elif kind == 7:  # a variable whose whole interval lies inside a run: it empties
        s, r = run(A1_WORDS[int(rng.integers(0, 3))])
        a = int(rng.integers(s, s + r))
        l[8], u[8] = lo + a, lo + int(rng.integers(a, s + r))
        singles()
    elif kind == 8:  # every variable assigned, no value twice, the XLessY records satisfied: the node ends True
        offs = [0, H] + [o for o in A1_OFFS[1:] if o < H]
        rest = [o for o in rng.permutation(np.arange(1, H)) if o not in offs]
        offs = np.array(offs + [int(o) for o in rest[: m - len(offs)]])
        offs[2:] = rng.permutation(offs[2:])
        offs[20:22] = np.sort(offs[20:22])
        offs[22:24] = np.sort(offs[22:24])
        l[:] = u[:] = lo + offs
    elif kind == 9:  # variable 22 alone holds the hull's upper end and x22 < x23 + 1 brings it to bit 126: a hull of 128 or 129 values comes under the mask
        u[1:] = lo + 126
        u[22] = lo + H
        l[1], l[22] = lo + H - 12, lo + 100
        b = A1_WORDS[int(rng.integers(0, 3))]
        for i in range(3):
            l[4 + i] = u[4 + i] = lo + b - 1 + i
        taken.update(range(b - 1, b + 2))
        l[8], u[8] = lo + b - 1, lo + H - 4
        singles()
    else:  # a mix: a run, singles, a few short intervals
        run(A1_WORDS[int(rng.integers(0, 3))])
        singles(0.8)
        for v in range(16, 20):
            a = int(rng.integers(0, H - 3))
            l[v], u[v] = lo + a, lo + min(H, a + int(rng.integers(1, 4)))
    return l, u


@functools.lru_cache(maxsize=None)
def a1_case():
    rng = splitmix64(4101)
    vs, cs = M.VStore(), M.CStore()
    xs = [vs.alloc((-130, 134)) for _ in range(A1_M)]
    cs.alloc(M.XLessY(xs[20], xs[21]))
    cs.alloc(M.Distinct(xs))
    cs.alloc(M.XLessY(xs[22], M.Addition(xs[23], 1)))
    cs.alloc(M.XLessY(xs[21], M.Addition(xs[22], 400)))
    rows = [_a1_row(rng, H, lo, k % 11, turn) for H in A1_HULLS for turn, lo in enumerate(A1_LOS) for k in range(A1_PER)]
    L, U = (np.stack([r[i] for r in rows]).astype(np.int32) for i in (0, 1))
    unit = list(range(A1_M))
    base = L[:, unit].min(axis=1)

    def crosses(b):
        def pred(ref):
            lb, ub, _, st = ref
            stay = (st != M.FALSE) & (lb[:, unit].min(axis=1) == base)
            up = ((L < (base + b)[:, None]) & (lb >= (base + b)[:, None])).any(axis=1)
            down = ((U >= (base + b)[:, None]) & (ub < (base + b)[:, None])).any(axis=1)
            return bool((stay & up).any() and (stay & down).any() and (stay & (up | down) & (hull(L, U, unit) <= 127)).any())
        return pred

    def duplicate(off):
        def pred(ref):  # under the mask from the first round (a hull of 127 at most), two assigned variables on that bit: the node fails
            twice = ((L == U) & (L == (base + off)[:, None])).sum(axis=1) >= 2
            return bool((twice & (hull(L, U, unit) <= 127) & (ref[3] == M.FALSE)).any()) and bool((ref[3][twice] == M.FALSE).all())
        return pred

    expect = {
        "a duplicate at bit 0": duplicate(0), "a duplicate at bit 64": duplicate(64), "a duplicate at bit 127": duplicate(127),
        "every (hull, lo) combination": lambda ref: set(zip(hull(L, U, unit).tolist(), base.tolist())) == {(h, lo) for h in A1_HULLS for lo in A1_LOS},
        "a bound crosses bits 31|32": crosses(32), "a bound crosses bits 63|64": crosses(64), "a bound crosses bits 95|96": crosses(96),
        "False, Unknown and True": ALL_STATUSES,
        "bounds within +-1000": lambda ref: bool(np.abs(L).max() <= 1000 and np.abs(U).max() <= 1000),
        "a hull of 128 or more comes under the mask": lambda ref: bool(((ref[3] != M.FALSE) & (hull(L, U, unit) >= 128) & (hull(ref[0], ref[1], unit) <= 127)).any()),
    }
    return ("A1",) + frozen((len(vs), cs.lower(len(vs)), L, U)) + (None, expect)


# ------------------------------------------------------------------------------------------------------------- A2 a hull that shrinks
@functools.lru_cache(maxsize=None)
def a2_case(low):
    """Eleven variables in (0, 40) and an outlier w in (0, 200) with w < x0 + 1 — or in (-160, 40) with x0 < w + 1: the unit's hull is
    200 on input, its pairs run in the first round, the outlier's bound comes in and the mask takes over."""
    rng = splitmix64(4201 + int(low))
    vs, cs = M.VStore(), M.CStore()
    xs = [vs.alloc((0, 40)) for _ in range(11)]
    w = vs.alloc((-160, 40) if low else (0, 200))
    cs.alloc(M.XLessY(xs[1], M.Addition(xs[2], 2)))
    cs.alloc(M.Distinct(xs + [w]))
    cs.alloc(M.XLessY(xs[0], M.Addition(w, 1)) if low else M.XLessY(w, M.Addition(xs[0], 1)))
    lb0, ub0 = vs.bounds()
    N = 72
    L, U = np.tile(lb0, (N, 1)).astype(np.int64), np.tile(ub0, (N, 1)).astype(np.int64)
    for k in range(N):
        end = 0 if not low else 40  # the values next to the end the outlier comes in at are the ones taken
        step = 1 if not low else -1
        n_asg = int(rng.integers(3, 8))
        who = 1 + rng.permutation(10)[:n_asg]
        vals = end + step * rng.permutation(9)[:n_asg]
        if rng.random() < 0.12:
            vals[-1] = vals[0]  # two variables, one value
        L[k, who] = U[k, who] = vals
        for v in range(11):
            if v in who:
                continue
            r = rng.random()
            if r < 0.6:    # a bound at the end where values are taken
                if low: U[k, v] = 40 - int(rng.integers(0, 3)); L[k, v] = int(rng.integers(0, 20))
                else: L[k, v] = int(rng.integers(0, 3)); U[k, v] = 40 - int(rng.integers(0, 20))
        if k % 4 == 3:  # the outlier already inside: the mask from the first round
            L[k, 11], U[k, 11] = 0, 40
    L, U = L.astype(np.int32), U.astype(np.int32)
    unit = list(range(12))

    def shrinks(ref):
        lb, ub, _, st = ref
        alive = st != M.FALSE
        hit = alive & (hull(L, U, unit) >= 128) & (hull(lb, ub, unit) <= 127) & ((lb[:, :11] != L[:, :11]) | (ub[:, :11] != U[:, :11])).any(axis=1)
        return 4 * int(hit.sum()) >= int(alive.sum()) > 0

    expect = {"the hull comes under the mask on a quarter of the nodes that do not fail": shrinks, "False and Unknown": _statuses(M.FALSE, M.UNKNOWN)}
    return ("A2-low" if low else "A2-high",) + frozen((len(vs), cs.lower(len(vs)), L, U)) + (None, expect)


# ------------------------------------------------------------------------------------------------------------------ A3 unit sizes
A3_DOM = {3: (0, 4), 63: (-3, 63), 64: (-3, 63)}
A3_VARS = {3: 5, 63: 65, 64: 64}


@functools.lru_cache(maxsize=None)
def a3_store(m):
    """(vs, cs, the pairs (a, b) of the records x_a < x_b).  m == 64: 64 variables, all in the unit: 2016 pair records and 16 more."""
    vs, cs = M.VStore(), M.CStore()
    V = A3_VARS[m]
    xs = [vs.alloc(A3_DOM[m]) for _ in range(V)]
    if m == 3:
        pairs = [(3, 4)]
        cs.alloc(M.XLessY(xs[3], xs[4]))
        cs.alloc(M.Distinct(xs[:3]))
        cs.alloc(M.XLessY(xs[0], M.Addition(xs[3], 5)))
        return vs, cs, pairs
    pairs = [(V - 1 - 2 * i, V - 2 - 2 * i) for i in range(10)]  # (with m == 63 the first two pairs hold the variables outside the unit)
    for a, b in pairs[:5]:
        cs.alloc(M.XLessY(xs[a], xs[b]))
    cs.alloc(M.Distinct(xs[:m]))
    for a, b in pairs[5:]:
        cs.alloc(M.XLessY(xs[a], xs[b]))
    for i in range(6):
        cs.alloc(M.XLessY(xs[i], M.Addition(xs[i + 7], 100)))
    return vs, cs, pairs


A3_KINDS = ("perm", "dup", "walk", "perm", "bad", "walk", "rand")


def a3_row(rng, m, kind):
    """perm: every variable assigned, no value twice, the XLessY records satisfied (True).  walk: the same with four variables of the unit
    (one if m == 3) opened again: they are walked to the values left free.  dup: the unit's first and last variable (lanes 0 and m - 1)
    with one value.  bad: lb > ub on input.  rand: assigned values that collide, and sub-boxes."""
    lo, hi = A3_DOM[m]
    V = A3_VARS[m]
    _, _, pairs = a3_store(m)
    vals = lo + rng.permutation(hi - lo + 1)[:V]
    for a, b in pairs:
        if vals[a] > vals[b]:
            vals[a], vals[b] = vals[b], vals[a]
    l, u = vals.copy(), vals.copy()
    if kind in ("walk", "bad"):
        for v in rng.permutation(m)[: 4 if m > 3 else 1]:
            l[v], u[v] = lo, hi
    if kind == "dup":
        l[m - 1] = u[m - 1] = vals[0]
    if kind == "bad":
        v = int(rng.integers(0, V))
        l[v], u[v] = vals[v] + 1, vals[v]
    if kind == "rand":
        p = rng.uniform(0.3, 0.95)
        for v in range(V):
            r = rng.random()
            if r < p:
                l[v] = u[v] = int(rng.integers(lo, hi + 1))
            elif r < p + 0.3:
                a = int(rng.integers(lo, hi + 1)); l[v], u[v] = a, int(rng.integers(a, hi + 1))
    return l, u


def a3_rows(seed, m, n):
    rng = splitmix64(seed)
    kinds = [A3_KINDS[k % len(A3_KINDS)] for k in range(n)]
    rows = [a3_row(rng, m, k) for k in kinds]
    return np.stack([r[0] for r in rows]).astype(np.int32), np.stack([r[1] for r in rows]).astype(np.int32), np.array(kinds)


@functools.lru_cache(maxsize=None)
def a3_case(m):
    vs, cs, _ = a3_store(m)
    V = len(vs)
    props = cs.lower(V)
    L, U, kinds = a3_rows(4300 + m, m, 70)

    def lowered(ref):
        grouped, left = alldiff_units(props, V)
        return len(grouped) == 1 and not left and grouped[0][1] == list(range(m)) and slot_count(props, V) == V

    expect = {
        f"the lowering groups one unit of {m} variables, lanes in variable order": lowered,
        "False, Unknown and True": ALL_STATUSES,
        "dup and bad nodes fail": lambda ref: bool((ref[3][(kinds == "dup") | (kinds == "bad")] == M.FALSE).all()),
        "walk nodes narrow": lambda ref: bool(((ref[3] == M.UNKNOWN) & (kinds == "walk") & ((ref[0] != L) | (ref[1] != U)).any(axis=1)).any()),
    }
    expect["permutation nodes are True"] = lambda ref: bool((kinds == "perm").any() and (ref[3][kinds == "perm"] == M.TRUE).all())
    if m == 64:
        expect["64 variables, 2016 pair records, at most 2048 records"] = lambda ref: V == 64 and int((props["group_kind"] == 2).sum()) == 2016 and 2016 < len(props) <= 2048
    return (f"A3-{m}",) + frozen((V, props, L, U)) + (None, expect)


# ------------------------------------------------------------------------------------------------------------------- A4 unit tables
@functools.lru_cache(maxsize=None)
def a4_case(n_ahead):
    """`n_ahead` one-record units, then nine Distinct units of 4 .. 8 of the 30 variables each (they share variables): the first eight
    are grouped, the ninth runs pair by pair.  Everything holds under a planted assignment.  `active` rows, by node: every unit; the
    first grouped unit off; the eighth; the ninth; all three; then three random rows with 15 % off."""
    rng = splitmix64(4400 + n_ahead)
    V, dom = 30, (0, 12)
    vs, cs = M.VStore(), M.CStore()
    xs = [vs.alloc(dom) for _ in range(V)]
    sol = rng.integers(dom[0], dom[1] + 1, V)
    for k in range(n_ahead):
        a, b = (int(t) for t in rng.choice(V, 2, replace=False))
        r = rng.random()
        if r < 0.15:
            cs.alloc(M.XLessY(xs[a], M.Constant(int(sol[a]) + 1 + int(rng.integers(0, 3)))))
        elif r < 0.7:
            cs.alloc(M.XLessY(xs[a], M.Addition(xs[b], int(sol[a] - sol[b]) + 1 + int(rng.integers(0, 4)))))
        else:
            c = int(rng.integers(-2, 3))
            cs.alloc(M.XNeqY(xs[a], M.Addition(xs[b], c + (1 if sol[a] == sol[b] + c else 0))))
    first = len(cs)
    for k in range(9):
        size, members = (6, 4, 7, 5, 8, 4, 5, 8, 7)[k], []
        for v in rng.permutation(V):
            if len(members) < size and all(sol[v] != sol[w] for w in members):
                members.append(int(v))
        assert len(members) == size
        cs.alloc(M.Distinct([xs[v] for v in members]))
    props = cs.lower(V)
    N = 120
    lb0, ub0 = vs.bounds()
    L1, U1 = random_nodes(4450 + n_ahead, lb0, ub0, N, sol, p_narrow=0.7)
    L, U = L1.copy(), U1.copy()
    for k in range(N):
        if k % 3 == 2:
            continue
        for v in range(V):  # many assigned variables: the units' masks have work; every twelfth node is the planted assignment itself (True)
            r = rng.random()
            if r < 0.45 or k % 12 == 0:
                L[k, v] = U[k, v] = sol[v] if (k % 3 == 0 or rng.random() < 0.8) else int(rng.integers(dom[0], dom[1] + 1))
    n_units = len(cs)
    act = random_active(4460 + n_ahead, N, n_units, p_off=0.15)
    full = orc.full_active(1, n_units)[0]
    bit = lambda u: np.uint64(1) << np.uint64(u & 63)
    for k in range(N):
        j = k % 8
        if j < 5:
            act[k] = full
            for u in {1: (first,), 2: (first + 7,), 3: (first + 8,), 4: (first, first + 7, first + 8)}.get(j, ()):
                act[k, u >> 6] &= ~bit(u)

    def tables(ref):
        grouped, left = alldiff_units(props, V)
        ids = [u for u, _ in grouped]
        edge = {31, 32} if n_ahead == 31 else {63, 64}
        return ids == list(range(first, first + 8)) and [u for u, _ in left] == [first + 8] and edge <= set(ids) and first == n_ahead

    def rows_matter(ref):
        full_ref = implicit_reference(f"A4-{n_ahead}")
        differs = (ref[3] != full_ref[3]) | (ref[0] != full_ref[0]).any(axis=1) | (ref[1] != full_ref[1]).any(axis=1)
        return all(differs[np.arange(N) % 8 == j].any() for j in (1, 2, 3, 4))

    expect = {"eight units grouped, the ninth not, ids on the word edge": tables, "False, Unknown and True": ALL_STATUSES,
              "switching the first, the eighth or the ninth Distinct off changes the answer": rows_matter}
    return (f"A4-{n_ahead}",) + frozen((V, props, L.astype(np.int32), U.astype(np.int32), act)) + (expect,)


# -------------------------------------------------------------------------------------------------------------------- B staging
B_DOM = (-9, 12)
B_SLOTS = (63, 64, 65, 127, 128)
B_UNITS = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 129)
B_NODES = 101
B_BATCHES = (1, 3, 4, 5, B_NODES)


def _planted(rng, sol, n_vars, p_const, p_tern):
    """One elementary propagator that holds under `sol`: x (kind) y + c or x (kind) y + z + c, y or z a Constant now and then."""
    lo, hi = B_DOM
    tern = rng.random() < p_tern
    v = [0, 0, 0]
    while len(set(v)) < 3:
        v = rng.integers(0, n_vars, 3).tolist()
    x, sx = M.Identity(v[0]), int(sol[v[0]])

    def operand(i):
        if rng.random() < p_const:
            c = int(rng.integers(lo, hi + 1))
            return None, c
        return M.Identity(v[i]), int(sol[v[i]])

    if not tern:
        r = rng.random()
        kind = M.NEQ if r < 0.35 else (M.EQ if r < 0.5 else M.LT)
        y, sy = operand(1)
        if y is None:  # against a Constant: its value is chosen, within the domain or one above, so that the planted assignment holds
            c = sx if kind == M.EQ else (int(rng.integers(sx + 1, hi + 2)) if kind == M.LT else (sy if sy != sx else sx + 1))
            return M.Elementary(kind, (x, M.Constant(c)))
        off = sx - sy if kind == M.EQ else (sx - sy + 1 + int(rng.integers(0, 6)) if kind == M.LT else int(rng.integers(-3, 4)))
        if kind == M.NEQ and sx == sy + off:
            off += 1
        return M.Elementary(kind, (x, M.Addition(y, off)))
    kind = (M.LT3, M.GT3, M.EQ3)[int(rng.integers(0, 3))]
    y, sy = M.Identity(v[1]), int(sol[v[1]])
    z, sz = operand(2)
    rest = sy + sz
    off = sx - rest if kind == M.EQ3 else (sx - rest + 1 + int(rng.integers(0, 6)) if kind == M.LT3 else sx - rest - 1 - int(rng.integers(0, 6)))
    return M.Elementary(kind, (x, M.Addition(y, off), M.Constant(sz) if z is None else z))


def staging_store(seed, n_vars0, n_recs, n_slots=None, n_units=None, p_const=0.15, p_tern=0.25):
    """(n_vars, props, sol).  `n_recs` planted propagators over `n_vars0` variables.  n_slots: further variables, each under one record
    x_new < x_old + c, bring the slot count (variables + interned constants) to exactly that.  n_units: the records are cut into that
    many runs, a run of several records a Conjunction; else every record is a unit."""
    rng = splitmix64(seed)
    sol = rng.integers(B_DOM[0], B_DOM[1] + 1, n_vars0)
    elems = [_planted(rng, sol, n_vars0, p_const, p_tern) for _ in range(n_recs)]
    n_vars = n_vars0
    if n_slots is not None:
        extra = n_slots - slot_count(M.lower_units(elems, n_vars0), n_vars0)
        assert extra >= 0, extra
        sol = np.concatenate([sol, rng.integers(B_DOM[0], B_DOM[1] + 1, extra)])
        for v in range(n_vars0, n_vars0 + extra):
            w = int(rng.integers(0, n_vars0))
            elems.insert(int(rng.integers(0, len(elems) + 1)), M.XLessY(M.Identity(v), M.Addition(M.Identity(w), int(sol[v] - sol[w]) + 1 + int(rng.integers(0, 4)))))
        n_vars += extra
    units = elems
    if n_units is not None:
        P = len(elems)
        cuts = [0] + sorted(int(c) for c in rng.choice(np.arange(1, P), n_units - 1, replace=False)) + [P]
        units = [elems[a] if b - a == 1 else M.Conjunction(tuple(elems[a:b])) for a, b in zip(cuts[:-1], cuts[1:])]
    return n_vars, M.lower_units(units, n_vars), sol


def staging_nodes(seed, n_vars, sol, n_units, n_nodes=B_NODES):
    """Boxes around the planted assignment (odd nodes) and arbitrary boxes (even nodes); `active` rows with 15 % of the units off, in
    every seventh node the last unit off, in every seventh the last unit alone."""
    lb0, ub0 = np.full(n_vars, B_DOM[0], np.int32), np.full(n_vars, B_DOM[1], np.int32)
    La, Ua = random_nodes(seed, lb0, ub0, n_nodes, sol, p_narrow=0.5)
    Lr, Ur = random_nodes(seed + 1, lb0, ub0, n_nodes, None, p_narrow=0.06)
    odd = (np.arange(n_nodes) % 2 == 1)[:, None]
    L, U = np.where(odd, La, Lr).astype(np.int32), np.where(odd, Ua, Ur).astype(np.int32)
    act = random_active(seed + 2, n_nodes, n_units, p_off=0.15)
    last = n_units - 1
    bit = np.uint64(1) << np.uint64(last & 63)
    for k in range(n_nodes):
        if k % 7 == 1:
            act[k, last >> 6] &= ~bit
        elif k % 7 == 2:
            act[k] = 0
            act[k, last >> 6] = bit
        elif k % 7 == 3:
            act[k, last >> 6] |= bit
    return L, U, act


def _staging_expect(n_vars, props, L, U, act, n_slots=None, n_units=None, n_recs=None):
    last = orc.OracleModel(n_vars, props).n_units - 1
    has = lambda a: ((a[:, last >> 6] >> np.uint64(last & 63)) & np.uint64(1)).astype(bool)
    drawn = ~np.isin(np.arange(len(act)) % 7, (1, 2, 3))
    expect = {
        "nodes that do not fail are narrowed": lambda ref: 5 * int(((ref[3] != M.FALSE) & ((ref[0] != L) | (ref[1] != U)).any(axis=1)).sum()) >= len(L),
        "False and Unknown": _statuses(M.FALSE, M.UNKNOWN),
        "fewer slots than variables + constants would be without interning, more than variables": lambda ref: n_vars < slot_count(props, n_vars),
        "the domain crosses zero": lambda ref: bool(L.min() < 0 < U.max()),
        "rows with the last unit off, and alone": lambda ref: bool((~has(act)).any() and (has(act) & (np.unpackbits(act.view(np.uint8), axis=1).sum(axis=1) == 1)).any()),
        "about 15 % of the bits off in the rows left as drawn": lambda ref: 0.1 < 1 - np.unpackbits(act[drawn].view(np.uint8), axis=1).sum() / (int(drawn.sum()) * (last + 1)) < 0.2,
        "the last unit is live on input on a node that does not fail": lambda ref: bool((has(act) & (ref[3] != M.FALSE)).any()),
    }
    if n_slots is not None:
        expect[f"exactly {n_slots} slots"] = lambda ref: slot_count(props, n_vars) == n_slots
    if n_units is not None:
        expect[f"exactly {n_units} units"] = lambda ref: orc.OracleModel(n_vars, props).n_units == n_units == last + 1
    if n_recs is not None:
        expect[f"exactly {n_recs} records"] = lambda ref: len(props) == n_recs
    return expect


@functools.lru_cache(maxsize=None)
def b_slots_case(S):
    n_vars, props, sol = staging_store(5100 + S, S - 26, 150 if S < 100 else 260, n_slots=S)
    L, U, act = staging_nodes(5200 + S, n_vars, sol, len(props))
    return (f"B-S{S}",) + frozen((n_vars, props, L, U, act)) + (_staging_expect(n_vars, props, L, U, act, n_slots=S),)


@functools.lru_cache(maxsize=None)
def b_units_case(n_units):
    n_vars, props, sol = staging_store(5300 + n_units, 40, max(40, n_units + 30), n_units=n_units)
    L, U, act = staging_nodes(5400 + n_units, n_vars, sol, n_units)
    return (f"B-U{n_units}",) + frozen((n_vars, props, L, U, act)) + (_staging_expect(n_vars, props, L, U, act, n_units=n_units),)


@functools.lru_cache(maxsize=None)
def b_limit_case(which):
    """The stores one step beyond the path's limits (pcp_api.hip): 129 slots, or 2049 records.  Small otherwise."""
    if which == "S129":
        n_vars, props, sol = staging_store(5501, 100, 90, n_slots=129)
        want = {"n_slots": 129}
    else:
        n_vars, props, sol = staging_store(5502, 60, 683, p_tern=0.1)  # 683 planted records, three times over: 2049 units of one record
        props = np.tile(props, 3)
        props["group"] = np.arange(len(props))
        want = {"n_recs": 2049}
    L, U, act = staging_nodes(5510 if which == "S129" else 5520, n_vars, sol, len(props), n_nodes=40)
    expect = _staging_expect(n_vars, props, L, U, act, **want)
    if which == "S129":
        expect["at most 2048 records"] = lambda ref: len(props) <= 2048
    else:
        expect["at most 128 slots"] = lambda ref: slot_count(props, n_vars) <= 128
    return (f"B-{which}",) + frozen((n_vars, props, L, U, act)) + (expect,)


# ------------------------------------------------------------------------------------------------------------------ C the node loop
C_NODES, C_PERIOD = 12288, 127


@functools.lru_cache(maxsize=None)
def c_case():
    """The 127 base rows over the 64-variable store of A3 (kinds in the order of A3_KINDS: True, False, Unknown next to each other);
    c_expand() makes the 12288 rows of the launch and of the expected result from them.  (127, a prime: the oracle's run on the base rows
    is the slow step of the test, and the period only has to keep a wavefront's consecutive nodes apart.)"""
    vs, cs, _ = a3_store(64)
    props = cs.lower(64)
    L, U, kinds = a3_rows(6100, 64, C_PERIOD)

    def mixed(ref):
        share = np.bincount(ref[3], minlength=3) / len(ref[3])
        return bool((share > 0).all() and share.max() <= 0.6)

    def neighbours(ref):
        st = ref[3]
        return all((((st[:-1] == a) & (st[1:] == b)) | ((st[:-1] == b) & (st[1:] == a))).any() for a in range(3) for b in range(a))

    expect = {"all three statuses, none above 60 %": mixed, "every status next to every other": neighbours,
              "distinct base rows": lambda ref: len({(l.tobytes(), u.tobytes()) for l, u in zip(L, U)}) == C_PERIOD,
              "lb > ub on input and duplicates": lambda ref: bool((L > U).any() and (kinds == "dup").any())}
    return ("C",) + frozen((64, props, L, U)) + (None, expect)


def c_expand(a):
    return a[np.arange(C_NODES) % C_PERIOD]


# -------------------------------------------------------------------------------------------------------------------- D node units
D_COUNTS = (0, 1, 63, 64, 65, 70)


def unary(var, kind, value, const_first=False):
    """One pcp_prop over a variable and Constant(value), in either operand order (as test_node_units._unary)."""
    p = np.zeros(1, dtype=M.PROP_DTYPE)
    p["kind"] = kind
    p["var"][0] = [M.PCP_CONST, var, M.PCP_NOVAR] if const_first else [var, M.PCP_CONST, M.PCP_NOVAR]
    p["off"][0] = [value, 0, 0] if const_first else [0, value, 0]
    return p


def with_units(props, extra):
    """The model's rows followed by a node's own, each a unit of its own (Store::alloc order)."""
    if not len(extra):
        return props
    e = extra.copy()
    e["group"] = np.arange(len(e)) + int(props["group"].max()) + 1
    return np.concatenate([props, e])


@functools.lru_cache(maxsize=None)
def d_case():
    """N-queens 8 with ONE Distinct (grouped).  The nodes are Unknown fixpoints of the oracle's search, each six times: with 0, 1, 63, 64,
    65 and 70 propagators of its own, in random order — x != v at a bound (the bound moves), x != v inside (kept: the node stays
    Unknown), x != v outside and x < c / c < x beyond the domain (entailed at once), a few x < c / c < x that cut, and repeats of
    all of these, several per variable.  Returns the case and the list of the nodes' propagator tables."""
    rng = splitmix64(7100)
    n = 8
    vs, cs = M.nqueens(n, "global")
    props = cs.lower(n)
    om = orc.OracleModel(n, props)
    lb0, ub0 = vs.bounds()
    _, _, rec, _ = om.search(lb0, ub0, all_solutions=True, node_limit=60, max_records=60)
    unk = rec["status"] == M.UNKNOWN
    PL, PU = rec["lb_out"][unk][:10], rec["ub_out"][unk][:10]
    rows_l, rows_u, units = [], [], []
    for i in range(len(PL)):
        open_vars = [v for v in range(n) if PL[i, v] < PU[i, v]]
        for cnt in D_COUNTS:
            ps = []
            cutters = rng.permutation(open_vars)[: min(cnt, int(rng.integers(1, 4)))]  # one to three propagators that act, each on a variable of its own
            for x in cutters:
                x, l, u = int(x), int(PL[i, x]), int(PU[i, x])
                r, first = rng.random(), bool(rng.integers(0, 2))
                if r < 0.5:
                    ps.append(unary(x, M.NEQ, l if rng.random() < 0.5 else u, first))                       # at a bound: it moves
                elif r < 0.75 and u - l >= 2:
                    ps.append(unary(x, M.NEQ, int(rng.integers(l + 1, u)), first))                            # inside: kept
                else:
                    ps.append(unary(x, M.LT, u) if rng.random() < 0.5 else unary(x, M.LT, l, True))          # x < u | l < x
            n_cut = len(ps)
            while len(ps) < cnt:  # the others are entailed at once, or keep an inside value of a variable that no cutter touches
                x = int(rng.integers(0, n))
                l, u = int(PL[i, x]), int(PU[i, x])
                r, first = rng.random(), bool(rng.integers(0, 2))
                if r < 0.45:
                    ps.append(unary(x, M.NEQ, int(rng.choice([l - 1, u + 1, 0, n + 1, 20, -7])), first))    # outside
                elif r < 0.7:
                    ps.append(unary(x, M.LT, u + 1 + int(rng.integers(0, 3))) if rng.random() < 0.5 else unary(x, M.LT, l - 1 - int(rng.integers(0, 3)), True))
                elif r < 0.8 and u - l >= 2 and x not in cutters:
                    ps.append(unary(x, M.NEQ, int(rng.integers(l + 1, u)), first))                            # inside
                elif len(ps) > n_cut:
                    ps.append(ps[int(rng.integers(n_cut, len(ps)))].copy())                                   # one of these again
            order = rng.permutation(cnt)
            if cnt > 64:  # a propagator that acts sits behind the 64th: the lane-strided loop's second trip carries it
                k = int(np.nonzero(order == 0)[0][0])
                order[k], order[cnt - 1] = order[cnt - 1], order[k]
            units.append(np.concatenate([ps[k] for k in order]) if cnt else np.zeros(0, dtype=M.PROP_DTYPE))
            rows_l.append(PL[i]); rows_u.append(PU[i])
    L, U = np.stack(rows_l).astype(np.int32), np.stack(rows_u).astype(np.int32)
    counts = np.array([len(u) for u in units])

    def kept(ref):
        base = orc.OracleModel(n, props).consistency(L, U, None)
        moved = (ref[0] != base[0]).any(axis=1) | (ref[1] != base[1]).any(axis=1)
        return bool(((counts >= 64) & (ref[3] == M.UNKNOWN) & moved).any())

    def second_trip(ref):
        # a node of 65 or 70 propagators whose answer changes when the ones past the 64th are dropped
        for i in np.nonzero(counts > 64)[0]:
            cut = orc.OracleModel(n, with_units(props, units[i][:64])).consistency(L[i : i + 1], U[i : i + 1], None)
            if cut[3][0] != ref[3][i] or not np.array_equal(cut[0][0], ref[0][i]) or not np.array_equal(cut[1][0], ref[1][i]):
                return True
        return False

    expect = {
        "the store has a grouped unit": lambda ref: [vs_ for _, vs_ in alldiff_units(props, n)[0]] == [list(range(n))],
        "a node of 64 or more propagators ends Unknown on a fixpoint of its own": kept,
        "a propagator past the 64th matters": second_trip,
        "every count": lambda ref: set(counts.tolist()) == set(D_COUNTS),
        "False and Unknown": _statuses(M.FALSE, M.UNKNOWN),
    }
    return ("D",) + frozen((n, props, L, U)) + (None, expect), units


@functools.lru_cache(maxsize=None)
def d_reference():
    """(lb, ub, None, status): every node against the oracle over the model plus that node's propagators."""
    (_, n, props, L, U, _, _), units = d_case()
    out = [orc.OracleModel(n, with_units(props, units[i])).consistency(L[i : i + 1], U[i : i + 1], None) for i in range(len(L))]
    return frozen((np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), None, np.concatenate([o[3] for o in out])))


CASES = {"A1": a1_case, "A2-high": lambda: a2_case(False), "A2-low": lambda: a2_case(True)}
CASES.update({f"A3-{m}": functools.partial(a3_case, m) for m in (3, 63, 64)})
CASES.update({f"A4-{k}": functools.partial(a4_case, k) for k in (31, 63)})
CASES.update({f"B-S{s}": functools.partial(b_slots_case, s) for s in B_SLOTS})
CASES.update({f"B-U{u}": functools.partial(b_units_case, u) for u in B_UNITS})
CASES.update({f"B-{w}": functools.partial(b_limit_case, w) for w in ("S129", "P2049")})
CASES["C"] = c_case
DISTINCT_CASES = ("A1", "A2-high", "A2-low", "A3-3", "A3-63", "A3-64", "A4-31", "A4-63")
LIMIT_CASES = ("B-S129", "B-P2049")
