"""What the tests of the set solution sink share (test_set_forest_sink_cpu.py, test_set_forest_sink_gpu.py; pcp_set_solution_sink_set): the
models, for each a brute-force solution set computed in plain Python from the constraints themselves over the hull (never through the
engine or the oracle), the restatement of the reference's search loop (setform_forest_ref.reference_search) made to keep the SETS of its
True nodes, and the checks a returned set of products must pass.  Every model has at most 6 variables and a hull of at most 8 values per
variable.  Results are computed once per process and never modified.  TEST INFRASTRUCTURE."""
import functools
import itertools

import numpy as np

from pcp_amd import model as M

import setform_cases as SC
import setform_forest_ref as R

BRANCHERS = R.BRANCHERS
# name -> (set_words, base = the hull's lower bound, hull's upper bound, the store has formula units)
SHAPE = {"rec4": (1, 0, 5, False), "rec2w": (2, -3, 66, False), "rec3w": (3, -3, 66, False), "form4": (1, 0, 4, True),
         "sched4": (1, 0, 7, True), "queens6": (1, 1, 6, False)}
MODELS = tuple(SHAPE)
# copy_node's two paths: a row of n_vars x set_words words goes 16 bytes at a time when that count is even (rows of a sink are then 16-byte
# aligned too), word by word when it is odd — rec2w (6 words) against rec3w (9 words, every odd row misaligned as well)
EVEN_ROWS, ODD_ROWS = ("rec4", "rec2w", "form4", "queens6"), ("rec3w", "sched4")


@functools.lru_cache(maxsize=None)
def build(name):
    """(vs, cs) of the model."""
    vs, cs = M.VStore(), M.CStore()
    if name == "rec4":  # the store test_forest_sink_gpu.py uses for its refusals
        x = [vs.alloc((0, 5)) for _ in range(4)]
        cs.alloc(M.XNeqY(x[0], x[1]))
        cs.alloc(M.XLessY(x[2], x[3]))
    elif name in ("rec2w", "rec3w"):
        # a negative base (the declared hull starts at -3), one variable straddling words 0 and 1.  The domains themselves stay non-negative:
        # MiddleVal truncates toward zero, so BinarySplit on [-1, 0] branches on x <= 0 and never ends — in the reference as on the device
        a, b, c = vs.alloc((0, 5)), vs.alloc((0, 5)), vs.alloc((60, 66))
        cs.alloc(M.XNeqY(a, b))
        cs.alloc(M.XLessY(M.Addition(a, 60), c))
    elif name == "form4":
        x, y, z, b = vs.alloc((0, 4)), vs.alloc((0, 4)), vs.alloc((0, 3)), vs.alloc((0, 1))
        cs.alloc(M.Or((M.XLessY(x, y), M.XEqY(x, M.Addition(z, 1)))))
        cs.alloc(M.equivalence(M.Boolean(b), M.XLessY(y, z)))
    elif name == "sched4":
        return R.schedule(R.DUR4, 8)[:2]
    elif name == "queens6":
        return M.nqueens(6)
    else:
        raise KeyError(name)
    return vs, cs


def satisfies(name, p):
    """The model's constraints on the point p, restated by hand."""
    if name == "rec4":
        return p[0] != p[1] and p[2] < p[3]
    if name in ("rec2w", "rec3w"):
        return p[0] != p[1] and p[0] + 60 < p[2]
    if name == "form4":
        x, y, z, b = p
        return (x < y or x == z + 1) and ((b == 1) == (y < z))
    if name == "sched4":
        return R.schedule_is_valid(p, R.DUR4)
    n = len(p)
    return all(p[i] != p[j] and abs(p[i] - p[j]) != j - i for i in range(n) for j in range(i + 1, n))


@functools.lru_cache(maxsize=None)
def brute(name):
    """The model's solutions as a frozenset of full assignments: every integer point of the hull that satisfies the constraints."""
    vs, _ = build(name)
    lb, ub = vs.bounds()
    assert len(lb) <= 6 and (np.asarray(ub) - np.asarray(lb) < 8).all()
    return frozenset(p for p in itertools.product(*[range(int(l), int(u) + 1) for l, u in zip(lb, ub)]) if satisfies(name, p))


def root_bits(name):
    """[V, set_words] uint64: the hull's sets."""
    vs, _ = build(name)
    sw, base, _, _ = SHAPE[name]
    return SC.hull_sets(vs, sw, base)


def members(row, base):
    """The values of each variable's set in a [V, set_words] uint64 row: a list of lists."""
    out = []
    for words in np.asarray(row, np.uint64):
        vals = []
        for k, w in enumerate(words):
            w = int(w)
            vals += [base + 64 * k + b for b in range(64) if (w >> b) & 1]
        out.append(vals)
    return out


class _KeepSets:
    """An OracleModel whose consistency_set also keeps (status, sets) of every node it ran: reference_search keeps lower bounds only."""

    def __init__(self, om):
        self._om = om
        self.seen = []

    def __getattr__(self, k):
        return getattr(self._om, k)

    def consistency_set(self, bits, base):
        out = self._om.consistency_set(bits, base)
        self.seen.append((int(out[4][0]), np.array(out[2][0], np.uint64)))
        return out


@functools.lru_cache(maxsize=None)
def reference(name, brancher="split", val="middle", node_limit=0):
    """setform_forest_ref.reference_search on the model from its hull, keeping the True nodes' SETS: dict(nodes, solutions, failed, sets =
    [solutions, V, set_words] uint64 in the order found, statuses = every node's status in the order run)."""
    vs, cs = build(name)
    sw, base, _, _ = SHAPE[name]
    om = _KeepSets(SC.oracle_model(vs, cs))
    r = R.reference_search(om, root_bits(name), base, brancher, val, node_limit)
    true = [b for s, b in om.seen if s == M.TRUE]
    if node_limit and r["nodes"] >= node_limit and om.seen[-1][0] == M.TRUE:
        true = true[:-1]  # StopNode's limit node is no solution (stop_node.rs:55-62)
    assert len(true) == r["solutions"] == len(r["rows"])
    sets = np.stack(true) if true else np.zeros((0, len(vs), sw), np.uint64)
    sets.setflags(write=False)
    return {"nodes": r["nodes"], "solutions": r["solutions"], "failed": r["failed"], "sets": sets, "statuses": tuple(s for s, _ in om.seen)}


def counts_of(name, brancher="split", val="middle", node_limit=0):
    r = reference(name, brancher, val, node_limit)
    return r["nodes"], r["solutions"], r["failed"]


def limit_on_a_true_node(name, brancher="split", val="middle"):
    """The smallest node limit at which StopNode's last node is a True node with at least one counted solution before it."""
    st = reference(name, brancher, val)["statuses"]
    return next(n for n in range(2, len(st) + 1) if st[n - 1] == M.TRUE and M.TRUE in st[:n - 1])


def check_products(name, rows, complete=True):
    """Every row is a product of non-empty sets, every point of every product is a solution, no point is covered twice, and (complete)
    together they cover every solution.  Returns (products wider than one point, products with a set that has a hole)."""
    sols = brute(name)
    base = SHAPE[name][1]
    seen, wide, holes = set(), 0, 0
    rows = np.asarray(rows, np.uint64)
    assert rows.ndim == 3 and rows.shape[1:] == root_bits(name).shape, rows.shape
    for k, row in enumerate(rows):
        dom = members(row, base)
        assert all(dom), (name, k, dom)
        wide += int(any(len(d) > 1 for d in dom))
        holes += int(any(d[-1] - d[0] + 1 != len(d) for d in dom))
        for p in itertools.product(*dom):
            assert p in sols, (name, k, p)
            assert p not in seen, (name, k, p, "covered twice")
            seen.add(p)
    if complete:
        assert seen == sols, (name, len(seen), len(sols))
    return wide, holes


def multiset(rows):
    rows = np.asarray(rows, np.uint64)
    return sorted(tuple(int(x) for x in r.ravel()) for r in rows)
