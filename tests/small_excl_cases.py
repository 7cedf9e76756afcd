"""The cases of the small-store exclusion tests (test_small_excl_cpu.py, test_small_excl_gpu.py): pcp_propagate_device_small_excl — nodes of
a SMALL store of any plain model that carry value exclusions x != v of their own (Enumerate's right branches, enumerate.rs:54-59), optionally
under branch and bound (branch_and_bound.rs:64-84).  Two models: the 12-variable N-queens with one XLessY (not an all-XNeqY model) and
golomb_ruler(5, 11) (XEqYPlusZ, XLessY, one Distinct).  The judge of every node is the oracle with the node's XNeqY(x, Constant(v)) units
allocated behind the model's (Branch::distribute, branch.rs:36-55).  Also here: a scalar restatement of the kernel's exclusion sweep and of
its fold, which test_small_excl_cpu.py holds against the same judge.  TEST INFRASTRUCTURE."""
import functools

import numpy as np

from oracle import oracle as orc
from pcp_amd import model as M

NONE = {"min": (1 << 29), "max": -(1 << 29)}  # "no solution yet": +-(PCP_BOUND_MAX + 1)


# ---------------------------------------------------------------------------------------------------------------- models
@functools.lru_cache(maxsize=None)
def queens_lt():
    """(n_vars, props, lb0, ub0): N-queens-12 and x0 < x1 — the model pcp_propagate_device_excl refuses (tests/test_neq_excl.py)."""
    n = 12
    props = M.nqueens_props(n)
    lt = np.zeros(1, dtype=M.PROP_DTYPE)
    lt["kind"] = M.LT
    lt["var"][0] = [0, 1, M.PCP_NOVAR]
    lt["group"] = int(props["group"].max()) + 1
    return n, np.concatenate([props, lt]), np.ones(n, np.int32), np.full(n, n, np.int32)


@functools.lru_cache(maxsize=None)
def golomb(m=5, length=11):
    """(n_vars, props, lb0, ub0, objective variable) of model.golomb_ruler."""
    vs, cs, var = M.golomb_ruler(m, length)
    lb0, ub0 = vs.bounds()
    return len(vs), cs.lower(len(vs)), lb0, ub0, var


# ---------------------------------------------------------------------------------------------------------------- the judge
def units(ex):
    """A node's exclusions as pcp_prop rows: x != Constant(v) each."""
    p = np.zeros(len(ex), dtype=M.PROP_DTYPE)
    p["kind"] = M.NEQ
    p["var"][:] = [0, M.PCP_CONST, M.PCP_NOVAR]
    p["var"][:, 0] = [int(e[0]) for e in ex]
    p["off"][:, 1] = [int(e[1]) for e in ex]
    return p


def with_units(props, ex):
    if not len(ex):
        return props
    e = units(ex)
    e["group"] = np.arange(len(e)) + int(props["group"].max()) + 1
    return np.concatenate([props, e])


_MODELS, _JUDGED = {}, {}


def plain_model(n, props):
    key = (n, props.tobytes())
    if key not in _MODELS:
        _MODELS[key] = orc.OracleModel(n, props)
    return _MODELS[key]


def judge(n, props, L, U, ex):
    """(status, lb, ub) of ONE node under the oracle; computed once per distinct node, shared and never changed."""
    ex = [(int(a), int(b)) for a, b in ex]
    key = (n, props.tobytes(), L.tobytes(), U.tobytes(), tuple(ex))
    if key not in _JUDGED:
        m = orc.OracleModel(n, with_units(props, ex)) if ex else plain_model(n, props)
        r = m.consistency(L[None], U[None], None)
        _JUDGED[key] = (int(r[3][0]), r[0][0].copy(), r[1][0].copy())
    return _JUDGED[key]


def oracle_nodes(n, props, L, U, excl):
    """(lb, ub, status) of every node under the oracle, each with its own exclusions."""
    lb, ub, st = L.copy(), U.copy(), np.zeros(len(L), np.uint8)
    for i in range(len(L)):
        st[i], lb[i], ub[i] = judge(n, props, L[i], U[i], excl[i])
    return lb, ub, st


def csr(excl, lead=0):
    """(offsets [n + 1] starting at `lead`, entries [lead + m, 2]): `lead` junk entries in front make the batch a slice of a larger CSR."""
    off = np.zeros(len(excl) + 1, np.int32)
    off[1:] = np.cumsum([len(e) for e in excl])
    flat = np.array([list(p) for e in excl for p in e], np.int64).reshape(-1, 2).astype(np.int32)
    junk = np.tile(np.array([[0x7FFFFFFF, 0]], np.int32), (lead, 1))  # (a var >= n_vars: reading it would refuse a node)
    flat = np.concatenate([junk, flat])
    return off + lead, (flat if len(flat) else np.zeros((1, 2), np.int32))


# ---------------------------------------------------------------------------------------------------------------- the restatement
def sweep(lb, ub, ex):
    """One pass of the kernel's exclusion sweep over ONE node, entry by entry on the bounds as they stand (XNeqY(Identity(var),
    Constant(value)), x_neq_y.rs:82-93): returns (lb, ub, failed, open, steps) — `open`: an entry is not entailed on what the pass left."""
    lb, ub = lb.copy(), ub.copy()
    failed, steps = False, 0
    for x, k in ex:
        steps += 1
        if lb[x] == ub[x]:
            failed |= lb[x] == k
        elif k == lb[x]:
            lb[x] += 1
        elif k == ub[x]:
            ub[x] -= 1
    opened = any(lb[x] <= k <= ub[x] for x, k in ex)
    return lb, ub, failed, opened, steps


def fold(lb, ub, var, mode, best):
    """The kernel's fold of the incumbent into the objective's cell: (lb, ub, emptied) — an emptied node keeps its row."""
    lb, ub = lb.copy(), ub.copy()
    if mode == "min":
        if best - 1 < ub[var]:
            if best - 1 < lb[var]:
                return lb, ub, True
            ub[var] = best - 1
    elif best + 1 > lb[var]:
        if best + 1 > ub[var]:
            return lb, ub, True
        lb[var] = best + 1
    return lb, ub, False


def restated(n, props, L, U, ex):
    """(status, lb, ub) of one node: sweeps and the model's fixpoint (the oracle's, without the node's units) in turn until nothing moves."""
    om = plain_model(n, props)
    lb, ub = L.copy(), U.copy()
    while True:
        l1, u1, failed, opened, _ = sweep(lb, ub, ex)
        if failed:
            return 0, lb, ub
        r = om.consistency(l1[None], u1[None], None)
        if int(r[3][0]) == 0:
            return 0, lb, ub
        l2, u2 = r[0][0], r[1][0]
        if np.array_equal(l2, lb) and np.array_equal(u2, ub):
            return (2 if (opened or int(r[3][0]) == 2) else 1), lb, ub
        lb, ub = l2.copy(), u2.copy()


def bnb_expected(n, props, L, U, excl, var, mode, best):
    """What pcp_propagate_device_small_excl leaves with an objective: (lb, ub, status, emptied, best, improved, winner or None)."""
    lb, ub, st, emp = L.copy(), U.copy(), np.zeros(len(L), np.uint8), np.zeros(len(L), bool)
    for i in range(len(L)):
        fl, fu, emp[i] = fold(L[i], U[i], var, mode, best)
        if not emp[i]:
            st[i], lb[i], ub[i] = judge(n, props, fl, fu, excl[i])
    true = np.nonzero(st == 1)[0]
    win = None
    if len(true):
        vals = lb[true, var].astype(np.int64)
        w = int(true[vals.argmin() if mode == "min" else vals.argmax()])  # the first of equal values: the lowest index
        if (lb[w, var] < best) if mode == "min" else (lb[w, var] > best):
            win = w
    return lb, ub, st, emp, (int(lb[win, var]) if win is not None else best), (1 if win is not None else 0), win


# ---------------------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def parents(which):
    """Propagated nodes of the oracle's own DFS over the model: (n, props, Unknown rows (lb, ub), solution rows (lb))."""
    n, props, lb0, ub0 = (queens_lt() if which == "queens" else golomb()[:4])
    _, _, rec, _ = plain_model(n, props).search(lb0, ub0, all_solutions=True, node_limit=120, max_records=120)
    unk, sol = rec["status"] == 2, rec["status"] == 1
    return n, props, rec["lb_out"][unk], rec["ub_out"][unk], rec["lb_out"][sol]


ENTRY_KINDS = ("none", "at_lb", "at_ub", "interior", "outside", "assigned_same", "assigned_other", "dups", "badvar")


@functools.lru_cache(maxsize=None)
def entry_cases(which):
    """Per-entry cases on the model's Unknown nodes: (n, props, L, U, excl, kind)."""
    n, props, PL, PU, _ = parents(which)
    L, U, excl, kind = [], [], [], []
    for i in range(min(len(PL), 27)):
        l, u = PL[i], PU[i]
        size = u.astype(np.int64) - l + 1
        k = ENTRY_KINDS[i % len(ENTRY_KINDS)]
        xs, zs = np.nonzero(size >= 3)[0], np.nonzero(size == 1)[0]
        x = int(xs[i % len(xs)]) if len(xs) else None
        z = int(zs[i % len(zs)]) if len(zs) else None
        ex = None
        if k == "none":
            ex = []
        elif x is not None and k == "at_lb":
            ex = [(x, l[x])]
        elif x is not None and k == "at_ub":
            ex = [(x, u[x])]
        elif x is not None and k == "interior":
            ex = [(x, l[x] + 1)]
        elif x is not None and k == "outside":
            ex = [(x, u[x] + 5), (x, l[x] - 3)]
        elif z is not None and k == "assigned_same":
            ex = [(z, l[z])]
        elif z is not None and k == "assigned_other":
            ex = [(z, l[z] + 1)]
        elif x is not None and k == "dups":
            ex = [(x, l[x]), (x, l[x]), (x, u[x]), (x, l[x])]
        elif x is not None and k == "badvar":
            ex = [(x, l[x]), (n, 3)]
        if ex is None:
            k, ex = "none", []
        L.append(l); U.append(u); excl.append([(int(a), int(b)) for a, b in ex]); kind.append(k)
    return n, props, np.stack(L), np.stack(U), excl, np.array(kind)


SEAM_COUNTS = (0, 1, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def seam_cases():
    """Lane-stride and round seams on the queens model over rows (1, 100): nodes with 0, 1, 63, 64, 65 and 130 entries (seeded: variables and
    values drawn around the bounds, so that some sit at a bound, some inside, some outside), and the chain — 70 consecutive values from the
    lower bound of one variable, shuffled, which only ever fall one at a time."""
    n, props, _, _ = queens_lt()
    rng = np.random.default_rng(4801)
    lb, ub = np.ones(n, np.int32), np.full(n, 100, np.int32)
    excl = []
    for c in SEAM_COUNTS:
        xs = rng.integers(0, n, c)
        vs = np.where(rng.random(c) < 0.5, rng.integers(-1, 6, c), rng.integers(95, 103, c))
        excl.append([(int(a), int(b)) for a, b in zip(xs, vs)])
    chain = [(5, int(v)) for v in rng.permutation(np.arange(1, 71))]
    excl.append(chain)
    L, U = np.tile(lb, (len(excl), 1)), np.tile(ub, (len(excl), 1))
    return n, props, L, U, excl, len(excl) - 1


@functools.lru_cache(maxsize=None)
def alldiff_cases():
    """Entries on the variables of golomb's Distinct: every difference of two values or more loses both its bounds, on nodes where other
    differences are assigned — the 128-value mask and the exclusions narrow the same variables."""
    n, props, PL, PU, _ = parents("golomb")
    m = golomb()[4] + 1
    L, U, excl = [], [], []
    for i in range(min(len(PL), 8)):
        l, u = PL[i], PU[i]
        ex = [(d, b) for d in range(m, n) if u[d] > l[d] for b in (int(l[d]), int(u[d]))]
        L.append(l); U.append(u); excl.append(ex)
    return n, props, np.stack(L), np.stack(U), excl, m


@functools.lru_cache(maxsize=None)
def bnb_batch():
    """A batch for the fold and the reduce on golomb_ruler(5, 11): Unknown nodes, then solutions (every one of length 11: they tie), Unknown
    nodes again; a few nodes carry exclusions."""
    n, props, PL, PU, SOL = parents("golomb")
    var = golomb()[4]
    assert len(SOL) >= 2 and (SOL[:, var] == SOL[0, var]).all()
    L = np.concatenate([PL[:6], SOL[:2], PL[6:10]])
    U = np.concatenate([PU[:6], SOL[:2], PU[6:10]])
    excl = [[] for _ in range(len(L))]
    for i in (1, 4, 9):
        size = U[i].astype(np.int64) - L[i] + 1
        x = int(np.nonzero(size >= 2)[0][0])
        excl[i] = [(x, int(L[i, x])), (x, int(U[i, x]))]
    return n, props, np.ascontiguousarray(L), np.ascontiguousarray(U), excl, var
