"""The models of the small-store forest tests (test_small_forest_cpu.py, test_small_forest_gpu.py): Golomb rulers (model.golomb /
golomb_ruler, the lengths of tools/bnb_golomb.py), a Golomb ruler whose marks start at -3, N-queens-8, and stores of plain propagators
built with small_cases.py's builders — mixed kinds with a Sum view and an XEqYMulZ, two Distinct units, a Distinct whose values span more
than 128, one of exactly 64 variables, more than 64 units, exactly 128 slots, exactly 2048 records.  A model is (vs, cs): everything is
pushed with model.push_model, the oracle side is form_forest_cases.oracle_model.  TEST INFRASTRUCTURE."""
import functools

import numpy as np

from pcp_amd import model as M

import small_cases as SC
from util import splitmix64

LENGTH = {5: 20, 6: 30}   # tools/bnb_golomb.py
OPTIMUM = {5: 11, 6: 17}
NODE_LIMIT = 2000         # of the mixed-kind stores
MIXED_SEEDS = tuple(range(7100, 7106))


def golomb(m):
    """(vs, cs, objective variable) of model.golomb_ruler at tools/bnb_golomb.py's length."""
    return M.golomb_ruler(m, LENGTH[m])


def golomb_shifted(m, shift):
    """model.golomb with every mark moved by `shift`: marks in [shift, length + shift], the first one = shift."""
    length = LENGTH[m]
    vs, cs = M.VStore(), M.CStore()
    marks = [vs.alloc((shift, length + shift)) for _ in range(m)]
    cs.alloc(M.XEqY(marks[0], M.Constant(shift)))
    for i in range(m - 1):
        cs.alloc(M.XLessY(marks[i], marks[i + 1]))
    diffs = {}
    for i in range(m - 1):
        for j in range(i + 1, m):
            diffs[(i, j)] = vs.alloc((1, length))
            cs.alloc(M.XEqYPlusZ(marks[j], marks[i], diffs[(i, j)]))
    cs.alloc(M.Distinct(list(diffs.values())))
    cs.alloc(M.XLessY(diffs[(0, 1)], diffs[(m - 2, m - 1)]))
    return vs, cs


def is_ruler(row, m):
    """The marks row[:m] increase and all their pairwise differences are distinct."""
    marks = [int(x) for x in row[:m]]
    d = [marks[j] - marks[i] for i in range(m - 1) for j in range(i + 1, m)]
    return all(x > 0 for x in d) and len(set(d)) == len(d)


def _store(n_vars, dom, units):
    vs, cs = M.VStore(), M.CStore()
    for _ in range(n_vars):
        vs.alloc(dom)
    for u in units:
        cs.alloc(u)
    return vs, cs


DOM = (0, SC.B_DOM[1])  # the roots stay at or above zero: below it MiddleVal's truncation toward zero makes the left child of (-2, -1) its parent again


def mixed(seed):
    """Twelve variables in (0, 12) under 14 planted propagators of every binary and ternary kind, Constants among the operands,
    and — holding under the same planted assignment — a Sum view, an XEqYMulZ and a Distinct of four variables."""
    rng = splitmix64(seed)
    V = 12
    sol = rng.integers(DOM[0], DOM[1] + 1, V)
    I = M.Identity
    units = [SC._planted(rng, sol, V, 0.2, 0.4) for _ in range(14)]
    a, b, c = (int(x) for x in rng.permutation(V)[:3])
    units.insert(3, M.XLessY(I(a), M.Addition(M.Sum((I(b), I(c))), int(sol[a] - sol[b] - sol[c]) + 1 + int(rng.integers(0, 3)))))
    x, y, z = (int(v) for v in rng.permutation(V)[:3])
    # x + p = (y + q) * (z + r) with small factors, whatever the planted values are
    fy, fz = int(rng.integers(1, 4)), int(rng.integers(-2, 3))
    units.insert(8, M.XEqYMulZ(M.Addition(I(x), fy * fz - int(sol[x])), M.Addition(I(y), fy - int(sol[y])), M.Addition(I(z), fz - int(sol[z]))))
    ds = [int(v) for v in rng.permutation(V)]
    pick = []
    for v in ds:  # four variables whose planted values differ
        if all(sol[v] != sol[w] for w in pick):
            pick.append(v)
        if len(pick) == 4:
            break
    units.append(M.Distinct([I(v) for v in pick]))
    k = int(rng.integers(0, V))
    units.append(M.XLessY(I(k), M.Constant(int(sol[k]) + 1 + int(rng.integers(0, 3)))))  # (a Constant operand whatever the draws above gave)
    return _store(V, DOM, units)


def two_distincts():
    """Two Distinct units of six and five variables that share two, between ordinary records."""
    rng = splitmix64(7201)
    V = 10
    sol = rng.permutation(np.arange(1, 1 + V))
    I = M.Identity
    units = [SC._planted(rng, sol, V, 0.1, 0.3) for _ in range(4)]
    units.append(M.Distinct([I(v) for v in range(6)]))
    units += [SC._planted(rng, sol, V, 0.1, 0.3) for _ in range(3)]
    units.append(M.Distinct([I(v) for v in range(4, 9)]))
    units.append(M.XLessY(I(9), M.Addition(I(0), int(sol[9] - sol[0]) + 2)))
    return _store(V, DOM, units)


def wide_distinct():
    """small_cases.a2_case(False)'s store from its root: eleven variables in (0, 40) and an outlier in (0, 200) in one Distinct — the hull
    spans 201 values, the unit's pairs run, the outlier's bound comes in (w < x0 + 1) and the 128-value mask takes over inside the loop."""
    vs, cs = M.VStore(), M.CStore()
    xs = [vs.alloc((0, 40)) for _ in range(11)]
    w = vs.alloc((0, 200))
    cs.alloc(M.XLessY(xs[1], M.Addition(xs[2], 2)))
    cs.alloc(M.Distinct(xs + [w]))
    cs.alloc(M.XLessY(w, M.Addition(xs[0], 1)))
    assert np.array_equal(cs.lower(len(vs)), SC.a2_case(False)[2])
    return vs, cs


def distinct64():
    """small_cases.a3_store(64) — 64 variables, all of them in one Distinct, and 16 XLessY — from the root (0, 63): permutations."""
    _, cs, _ = SC.a3_store(64)
    vs = M.VStore()
    for _ in range(64):
        vs.alloc((0, 63))
    return vs, cs


class _Lowered:
    """A store given as its lowered table (small_cases.staging_store): what push_model needs of a CStore."""

    def __init__(self, props):
        self.props = props

    def pushes(self, n_vars, sums_out=None):
        return [("props", self.props)]

    def lower(self, n_vars):
        return self.props

    def __len__(self):
        return int(SC.unit_of_prop(self.props)[-1]) + 1


def _staged(n_vars, props, sol=None):
    """The root of a staged store: (0, 12); a variable whose planted value is negative is fixed to it, so the planted assignment stays."""
    vs = M.VStore()
    for v in range(n_vars):
        vs.alloc(DOM if sol is None or sol[v] >= 0 else (int(sol[v]), int(sol[v])))
    return vs, _Lowered(props)


def many_units():
    n_vars, props, sol = SC.staging_store(7301, 40, 100)
    return _staged(n_vars, props, sol)


def slots128():
    n_vars, props, sol = SC.staging_store(7302, 102, 260, n_slots=128)
    return _staged(n_vars, props, sol)


def recs2048():
    n_vars, props, sol = SC.staging_store(7303, 60, 64, p_tern=0.1)  # 64 planted records, 32 times over: 2048 units of one record
    props = np.tile(props, 32)
    props["group"] = np.arange(len(props))
    return _staged(n_vars, props, sol)


def slots129():
    _, n_vars, props, *_ = SC.b_limit_case("S129")
    return _staged(n_vars, props)


def recs2049():
    _, n_vars, props, *_ = SC.b_limit_case("P2049")
    return _staged(n_vars, props)


def queens8():
    return M.nqueens(8)


STORES = {"two-distincts": two_distincts, "wide-distinct": wide_distinct, "distinct64": distinct64, "many-units": many_units,
          "slots128": slots128, "recs2048": recs2048, **{f"mixed-{s}": functools.partial(mixed, s) for s in MIXED_SEEDS}}


@functools.lru_cache(maxsize=None)
def store(name):
    return STORES[name]()
