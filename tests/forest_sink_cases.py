"""What the tests of the solution sink share (test_forest_sink_cpu.py, test_forest_sink_gpu.py; pcp_solution_sink_set): the four models —
N-queens 6 and 8, a Golomb ruler of four marks capped at length 8, a three-task Cumulative schedule —, for each a brute-force solution
set computed in plain Python from the constraints themselves (never through the engine or the oracle), the checks a returned set of boxes
must pass against it, and a wrapper that makes the host-stepped search keep whole (lb, ub) rows of its True nodes.  TEST INFRASTRUCTURE."""
import functools
import itertools

import numpy as np

from pcp_amd import model as M

GOLOMB_M, GOLOMB_LENGTH = 4, 8
# the schedule: durations, resources, start window; capacity 3.  Tasks 0 and 1 (two units each) can never overlap, task 2 (one unit) fits next
# to either of them: once 0 and 1 are apart every unit is entailed whatever task 2 does — a True node that is a proper box
SCHED = ((2, 2, 1), (2, 2, 1), (0, 3))
CAPACITY = 3

# brute-force solution counts (test_forest_sink_cpu.py checks them against a fresh enumeration)
N_SOLUTIONS = {"queens6": 4, "queens8": 92, "golomb4": 8, "sched3": 24}
# ... and the complete BinarySplit tree of each from its root: (nodes, True nodes, failed, True nodes wider than one point)
SPLIT_TREE = {"queens6": (75, 4, 34, 0), "queens8": (779, 92, 298, 0), "golomb4": (21, 8, 3, 0), "sched3": (91, 21, 25, 3)}
KIND = {"queens6": "small", "queens8": "small", "golomb4": "small", "sched3": "form"}


@functools.lru_cache(maxsize=None)
def build(name):
    """(vs, cs) of the model."""
    if name.startswith("queens"):
        return M.nqueens(int(name[6:]))
    if name == "golomb4":
        vs, cs, _ = M.golomb_ruler(GOLOMB_M, GOLOMB_LENGTH)
        return vs, cs
    durations, resources, win = SCHED
    vs, cs = M.VStore(), M.CStore()
    starts = [vs.alloc(win) for _ in durations]
    cap = vs.alloc((CAPACITY, CAPACITY))
    M.Cumulative(starts, [M.Constant(d) for d in durations], [M.Constant(r) for r in resources], cap).join(vs, cs)
    return vs, cs


def root(name):
    vs, _ = build(name)
    lb0, ub0 = vs.bounds()
    return np.ascontiguousarray(lb0, np.int32), np.ascontiguousarray(ub0, np.int32)


@functools.lru_cache(maxsize=None)
def brute(name):
    """The model's solutions as a frozenset of full assignments (tuples over every variable of the store, in allocation order)."""
    out = set()
    if name.startswith("queens"):
        n = int(name[6:])
        for q in itertools.permutations(range(1, n + 1)):
            if all(abs(q[i] - q[j]) != j - i for i in range(n) for j in range(i + 1, n)):
                out.add(tuple(q))
    elif name == "golomb4":
        m, length = GOLOMB_M, GOLOMB_LENGTH
        pairs = [(i, j) for i in range(m - 1) for j in range(i + 1, m)]
        for rest in itertools.combinations(range(1, length + 1), m - 1):  # 0 = m_0 < m_1 < ..
            marks = (0,) + rest
            d = [marks[j] - marks[i] for i, j in pairs]
            if len(set(d)) == len(d) and d[pairs.index((0, 1))] < d[pairs.index((m - 2, m - 1))]:
                out.add(marks + tuple(d))
    else:
        durations, resources, win = SCHED
        n = len(durations)
        for s in itertools.product(range(win[0], win[1] + 1), repeat=n):
            aux, ok = [], True
            for j in range(n):  # Cumulative.join: per task j, per i != j a Boolean b = (s_i <= s_j < s_i + d_i) and r = b * r_i; c >= r_j + sum r
                load = resources[j]
                for i in range(n):
                    if i != j:
                        b = int(s[i] <= s[j] < s[i] + durations[i])
                        aux += [b, b * resources[i]]
                        load += b * resources[i]
                ok &= load <= CAPACITY
            if ok:
                out.add(tuple(s) + (CAPACITY,) + tuple(aux))
    return frozenset(out)


def points(lb, ub):
    """Every point of the box (lb, ub), as tuples."""
    return itertools.product(*[range(int(l), int(u) + 1) for l, u in zip(lb, ub)])


def check_boxes(name, lbs, ubs):
    """The boxes are non-empty, every point of every box is a solution, no point is covered twice, and together they cover every solution.
    Returns the number of boxes that are wider than one point."""
    sols = brute(name)
    seen, proper = set(), 0
    lbs, ubs = np.asarray(lbs), np.asarray(ubs)
    assert lbs.shape == ubs.shape and lbs.ndim == 2
    for k, (l, u) in enumerate(zip(lbs, ubs)):
        assert (l <= u).all(), (k, l, u)
        proper += int((l < u).any())
        for p in points(l, u):
            assert p in sols, (name, k, p)
            assert p not in seen, (name, k, p, "covered twice")
            seen.add(p)
    assert seen == sols, (name, len(seen), len(sols))
    return proper


def multiset(rows):
    return sorted(tuple(int(x) for x in r) for r in rows)


class KeepBoxes:
    """A context for pcp_amd.search.dfs / dfs_enumerate that passes everything through to ``ctx`` and keeps the (lb, ub) row of every node its
    propagate() reports True: the host-stepped search itself keeps lower bounds only."""

    def __init__(self, ctx):
        self._ctx = ctx
        self.boxes = []

    def __getattr__(self, k):
        return getattr(self._ctx, k)

    def propagate(self, lb, ub, active=None, want_stats=True):
        out = self._ctx.propagate(lb, ub, active, want_stats)
        for l, u, s in zip(out[0], out[1], out[3]):
            if s == M.TRUE:
                self.boxes.append((np.array(l, np.int32), np.array(u, np.int32)))
        return out


def stand_in(name):
    """The oracle-backed stand-in of engine.Context over the model: the one the CPU forest tests of its kind of store use."""
    vs, cs = build(name)
    if KIND[name] == "form":
        from form_forest_cases import FormulaOracleCtx
        return FormulaOracleCtx(vs, cs)
    from test_small_excl_cpu import SmallExclOracleCtx
    return SmallExclOracleCtx(len(vs), cs.lower(len(vs)))
