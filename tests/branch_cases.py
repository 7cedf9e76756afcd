"""Brancher<FirstSmallestVar, MiddleVal, BinarySplit> over Interval rows at its edges — TEST INFRASTRUCTURE shared by
test_branch_cases_cpu.py and test_branch_edges_gpu.py: the cases, and a scalar restatement of the brancher that shares no code with
pcp_amd.search.branch (plain Python integers, one row at a time):

* variable  first index among the variables of minimal size > 1           (first_smallest_var.rs:30-39)
* value     (lb + ub) / 2 truncated toward zero                           (middle_val.rs:25-27)
* children  `x <= v`, then `x > v`, folded into the bounds                (binary_split.rs:46-57)

A case is a batch of rows as the device brancher takes them: lb / ub [n, V] int32, status [n] uint8, `active` [n, words] uint64 or None,
n_units, and `claims`: what the case exists for, in a form test_branch_cases_cpu.py recomputes from the arrays.  Generators are pure
functions of fixed seeds.  numpy only; nothing here touches a GPU."""
import functools

import numpy as np

from pcp_amd import model as M

UNKNOWN, HULL = 2, 0xFE
NOVAR = 0xFFFFFFFF          # what the device writes as the hint of an Unknown row with nothing to split
CELL_MAX = 16383            # |bound| limit of the packed cell format
BOUND_MAX = (1 << 29) - 1   # |bound| limit of int32 rows (PCP_BOUND_MAX)
BLOCK = 256                 # threads of branch_kernel / branch_cells_kernel: variable v is read by thread v % 256 in iteration v // 256
SCAN_BLOCK = 1024           # threads of branch_scan_kernel: node i is read by thread i % 1024 in chunk i // 1024


# --------------------------------------------------------------------------------------------------------- the scalar reference
def ref_var(lb_row, ub_row):
    """FirstSmallestVar: the first index of minimal size > 1, or None when every variable is assigned (the reference panics)."""
    best, best_size = None, None
    for i, (a, b) in enumerate(zip(lb_row, ub_row)):
        size = int(b) - int(a) + 1
        if size > 1 and (best is None or size < best_size):
            best, best_size = i, size
    return best


def ref_middle(a, b):
    """MiddleVal: (a + b) / 2 with Rust's `/` on i32 — the quotient of the magnitudes, with the sign of the sum."""
    s = int(a) + int(b)
    q = abs(s) // 2
    return q if s >= 0 else -q


def ref_children(lb_row, ub_row):
    """(var, (lb, ub) of `x <= v`, (lb, ub) of `x > v`) as lists of ints; var None: nothing to split, both children are the parent."""
    l0, u0 = [int(x) for x in lb_row], [int(x) for x in ub_row]
    l1, u1 = list(l0), list(u0)
    var = ref_var(lb_row, ub_row)
    if var is not None:
        v = ref_middle(l0[var], u0[var])
        u0[var] = min(u0[var], v)
        l1[var] = max(l1[var], v + 1)
    return var, (l0, u0), (l1, u1)


def expected(lb, ub, status, active=None):
    """What the device brancher must write for the batch, in tree order (branch_reverse 0): child_lb / child_ub [k, V] int32, child_active
    [k, words] uint64 or None, dirty [k] uint32 (the variable branched on, NOVAR for a row with nothing to split) and counts =
    [n_children, n_true, n_false, n_unknown, n_other]."""
    n, V = lb.shape
    cl, cu, ca, cd = [], [], [], []
    tally = {0: 0, 1: 0, 2: 0, "other": 0}
    for i in range(n):
        st = int(status[i])
        tally[st if st <= UNKNOWN else "other"] += 1
        if st != UNKNOWN:
            continue
        var, left, right = ref_children(lb[i], ub[i])
        for l, u in (left, right):
            cl.append(l); cu.append(u); cd.append(NOVAR if var is None else var)
            if active is not None:
                ca.append(active[i])
    k = len(cl)
    return {"child_lb": np.array(cl, np.int64).reshape(k, V).astype(np.int32), "child_ub": np.array(cu, np.int64).reshape(k, V).astype(np.int32),
            "child_active": None if active is None else np.array(ca, np.uint64).reshape(k, active.shape[1]),
            "dirty": np.array(cd, np.uint32), "counts": [k, tally[1], tally[0], tally[2], tally["other"]]}


def units_model(n_vars, n_units):
    """n_units distinct binary units `x != y + c` over n_vars variables (no constants): a model whose `active` rows have
    ceil(n_units / 64) words.  The brancher never runs it."""
    props = np.zeros(n_units, dtype=M.PROP_DTYPE)
    props["var"][:] = M.PCP_NOVAR
    props["group"] = np.arange(n_units)
    props["kind"] = M.NEQ
    pairs = [(x, y) for x in range(n_vars) for y in range(n_vars) if x != y]
    assert n_units == 0 or pairs
    for r in range(n_units):
        x, y = pairs[r % len(pairs)]
        props[r]["var"][0], props[r]["var"][1], props[r]["off"][1] = x, y, r // len(pairs)
    return props


def _case(name, family, lb, ub, status, active=None, n_units=0, **claims):
    lb, ub = np.ascontiguousarray(lb, np.int32), np.ascontiguousarray(ub, np.int32)
    return {"name": name, "family": family, "lb": lb, "ub": ub, "status": np.ascontiguousarray(status, np.uint8),
            "active": active, "n_units": n_units, "claims": claims}


def fits_cells(case):
    """Rows whose every bound lies within +-16383 (a bool per row)."""
    return ((np.abs(case["lb"].astype(np.int64)) <= CELL_MAX) & (np.abs(case["ub"].astype(np.int64)) <= CELL_MAX)).all(axis=1)


# --------------------------------------------------------------------------------------------------------- 1. the scan
SCAN_V = 5
SCAN_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3100)
SCAN_PATTERNS = ("all_unknown", "no_unknown", "unknown_on_seams", "others_on_seams")


def seams(n):
    """The first and the last index of every 64-node span of [0, n) — a wavefront of the scan — which includes those of every 1024-node
    span, a chunk of its loop; the last span may be short, so n - 1 is one of them."""
    idx = {i for i in range(n) if i % 64 in (0, 63)} | {n - 1}
    return np.array(sorted(idx))


def _small_rows(rng, n, V, lo=-9, hi=9):
    """Rows of short domains inside [lo, hi], every one with a variable of two values or more."""
    L = rng.integers(lo, hi + 1, size=(n, V))
    U = L + rng.integers(0, 5, size=(n, V))
    free = rng.integers(0, V, size=n)
    U[np.arange(n), free] = np.maximum(U[np.arange(n), free], L[np.arange(n), free] + 1)
    return L.astype(np.int32), U.astype(np.int32)


def scan_case(n, pattern):
    rng = np.random.default_rng(5100 + 7 * n + SCAN_PATTERNS.index(pattern))
    lb, ub = _small_rows(rng, n, SCAN_V)
    others = np.array([0, 1, HULL], np.uint8)
    if pattern == "all_unknown":
        status = np.full(n, UNKNOWN, np.uint8)
    elif pattern == "no_unknown":
        status = others[rng.integers(0, 3, size=n)]
    else:
        status = np.array([0, 1, UNKNOWN, HULL], np.uint8)[rng.integers(0, 4, size=n)]
        s = seams(n)
        status[s] = UNKNOWN if pattern == "unknown_on_seams" else others[rng.integers(0, 3, size=len(s))]
    return _case(f"scan-{n}-{pattern}", "scan", lb, ub, status, n_nodes=n, pattern=pattern)


# --------------------------------------------------------------------------------------------------------- 2. the selection
SELECT_VS = (1, 2, 63, 64, 65, 255, 256, 257, 513, 1000)
UNIQUE_AT = (0, 63, 64, 255, 256)          # and V - 1
TIE_PAIRS = ((70, 300), (1, 256), (63, 64), (255, 511))  # and (0, V - 1): the lower index must win
BIG_SIZES = ((1 << 16) + 1, (1 << 30) - 1)


def select_case(V):
    """One batch: per row (lb, ub) and a claim — ("unique", i): variable i alone has the minimal size; ("one_free", i): every variable but
    i is assigned; ("tie", i, j): i < j share the minimal size, everything else is larger; ("assigned_first", i): variables of size 1 sit in
    front of the minimum at i; ("big", i, j): the only candidates are i of size 2^30 - 1 and j > i of size 2^16 + 1 (V = 1: i alone)."""
    rng = np.random.default_rng(5200 + V)
    rows, claims = [], []

    def wide():  # sizes 5 .. 9: larger than any minimum placed below
        L = rng.integers(-9, 1, size=V)
        return L, L + rng.integers(4, 9, size=V)

    for i in sorted({x for x in UNIQUE_AT if x < V} | {V - 1}):
        L, U = wide()
        U[i] = L[i] + 1
        rows.append((L, U)); claims.append(("unique", i))
    i = V // 2
    L = rng.integers(-9, 10, size=V); U = L.copy()
    U[i] = L[i] + 3
    rows.append((L, U)); claims.append(("one_free", i))
    for i, j in sorted({p for p in TIE_PAIRS if p[1] < V} | ({(0, V - 1)} if V >= 2 else set())):
        L, U = wide()
        U[i], U[j] = L[i] + 2, L[j] + 2
        rows.append((L, U)); claims.append(("tie", i, j))
    if V >= 2:
        L, U = wide()
        i = V - 1
        U[:i] = np.where(rng.random(i) < 0.5, L[:i], U[:i])
        U[0] = L[0]  # size 1 at the first index, the minimum of the rest at the last
        U[i] = L[i] + 1
        rows.append((L, U)); claims.append(("assigned_first", i))
    L = rng.integers(-9, 10, size=V).astype(np.int64); U = L.copy()
    i, j = (0, None) if V == 1 else (V // 3, V - 1)
    L[i], U[i] = -BOUND_MAX, BOUND_MAX
    if j is not None:
        L[j], U[j] = -(1 << 15), 1 << 15
    rows.append((L, U)); claims.append(("big", i, j))
    lb, ub = np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int64)
    return _case(f"select-{V}", "select", lb, ub, np.full(len(rows), UNKNOWN, np.uint8), V=V, rows=claims)


# --------------------------------------------------------------------------------------------------------- 3. signed MiddleVal
MIDDLE_WINDOWS = {"small": [(-6, 6)],
                  "cell_edge": [(-CELL_MAX, -CELL_MAX + 6), (CELL_MAX - 6, CELL_MAX)],
                  "row_edge": [(-BOUND_MAX, -BOUND_MAX + 6), (BOUND_MAX - 6, BOUND_MAX)]}
MIDDLE_SPANS = {"small": [], "cell_edge": [(-CELL_MAX, CELL_MAX), (-CELL_MAX, CELL_MAX - 1), (-CELL_MAX + 1, CELL_MAX - 2)],
                "row_edge": [(-BOUND_MAX, BOUND_MAX), (-BOUND_MAX, BOUND_MAX - 1), (-BOUND_MAX + 1, BOUND_MAX - 2)]}


def middle_case(which):
    """V = 3, two variables assigned; the third (at position row % 3) takes every [a, b], a < b, of each window, and the spans that cross
    zero from edge to edge."""
    doms = [(a, b) for lo, hi in MIDDLE_WINDOWS[which] for a in range(lo, hi + 1) for b in range(a + 1, hi + 1)] + MIDDLE_SPANS[which]
    lb = np.zeros((len(doms), 3), np.int64); ub = np.zeros((len(doms), 3), np.int64)
    for r, (a, b) in enumerate(doms):
        lb[r] = ub[r] = [a, b, 0]  # the assigned ones hold values from the same range
        lb[r, r % 3], ub[r, r % 3] = a, b
    return _case(f"middle-{which}", "middle", lb, ub, np.full(len(doms), UNKNOWN, np.uint8), which=which, doms=doms)


# --------------------------------------------------------------------------------------------------------- 4. `active` rows
ACTIVE_UNITS = (1, 64, 65, 320, 16450)
ACTIVE_WORDS = (1, 1, 2, 5, 258)
ACTIVE_V, ACTIVE_NODES = 9, 130


def active_case(n_units):
    rng = np.random.default_rng(5400 + n_units)
    lb, ub = _small_rows(rng, ACTIVE_NODES, ACTIVE_V)
    status = np.array([0, 1, UNKNOWN, UNKNOWN, UNKNOWN, HULL], np.uint8)[rng.integers(0, 6, size=ACTIVE_NODES)]
    words = (n_units + 63) // 64
    act = np.frombuffer(rng.bytes(8 * ACTIVE_NODES * words), np.uint64).reshape(ACTIVE_NODES, words).copy()
    if n_units % 64:  # zero tail bits
        act[:, -1] &= np.uint64((1 << (n_units % 64)) - 1)
    return _case(f"active-{n_units}", "active", lb, ub, status, act, n_units, words=words)


# --------------------------------------------------------------------------------------------------------- 5. nothing to split
def nosplit_case():
    """Seven rows under status Unknown; the one in the middle has every variable assigned."""
    rng = np.random.default_rng(5500)
    lb, ub = _small_rows(rng, 7, 4)
    ub[3] = lb[3]
    return _case("nosplit", "nosplit", lb, ub, np.full(7, UNKNOWN, np.uint8), row=3)


FAMILY_SIZES = {"scan": len(SCAN_SIZES) * len(SCAN_PATTERNS), "select": len(SELECT_VS), "middle": len(MIDDLE_WINDOWS),
                "active": len(ACTIVE_UNITS), "nosplit": 1}


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case, the row with nothing to split last.  Built once and shared: the tests must not write into the arrays."""
    cases = [scan_case(n, p) for n in SCAN_SIZES for p in SCAN_PATTERNS]
    cases += [select_case(V) for V in SELECT_VS]
    cases += [middle_case(w) for w in MIDDLE_WINDOWS]
    cases += [active_case(u) for u in ACTIVE_UNITS]
    cases.append(nosplit_case())
    for c in cases:
        for k in ("lb", "ub", "status", "active"):
            if c[k] is not None:
                c[k].setflags(write=False)
    return tuple(cases)


CASE_NAMES = ([f"scan-{n}-{p}" for n in SCAN_SIZES for p in SCAN_PATTERNS] + [f"select-{V}" for V in SELECT_VS] +
              [f"middle-{w}" for w in MIDDLE_WINDOWS] + [f"active-{u}" for u in ACTIVE_UNITS] + ["nosplit"])


def case_by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def expected_by_name(name):
    c = case_by_name(name)
    return expected(c["lb"], c["ub"], c["status"], c["active"])
