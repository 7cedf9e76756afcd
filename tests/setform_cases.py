"""Shared cases of the set-mode formula tests (test_setform_cpu.py, test_setform_gpu.py): stores of formula units over IntervalSet
domains, their random nodes, and the oracle's answers — computed once per process and never modified."""
import functools

import numpy as np

from oracle import oracle as orc
from pcp_amd import model as M

from test_reified import random_formula_store
from test_set_mode import bits_of, random_sets

SEEDS = range(40)
NODES_PER_STORE = 8


def oracle_model(vs, cs):
    om = orc.OracleModel(len(vs))
    M.push_model(om, cs, len(vs))
    return om


def hull_sets(vs, sw, base):
    lb, ub = vs.bounds()
    return M.interval_bits(lb, ub, sw, base)


@functools.lru_cache(maxsize=None)
def random_case(seed, dom=(0, 6), sw=1, base=0, n_nodes=NODES_PER_STORE, n_units=10):
    """(vs, cs, bits [n_nodes, V, sw]) of one random formula store (12 variables, about 10 units) and its random set-valued nodes."""
    vs, cs = random_formula_store(seed, n_units=n_units, dom=dom)
    lb, ub = vs.bounds()
    bits = random_sets(seed + 1000, lb, ub, n_nodes, sw, base, p_keep=0.8)
    bits.setflags(write=False)
    return vs, cs, bits


@functools.lru_cache(maxsize=None)
def random_reference(seed, dom=(0, 6), sw=1, base=0, n_nodes=NODES_PER_STORE, n_units=10):
    """The oracle's set-mode fixpoints of random_case's nodes, every unit active: (lb, ub, bits, active, status)."""
    vs, cs, bits = random_case(seed, dom, sw, base, n_nodes, n_units)
    ref = oracle_model(vs, cs).consistency_set(bits, base)[:5]
    for a in ref:
        a.setflags(write=False)
    return ref


def hand_or_eq_bool():
    """x = {1, 3, 5}, y = {2, 4}, b = {0, 1}; one unit Or(XEqY(x, y), Boolean(b))."""
    vs, cs = M.VStore(), M.CStore()
    x, y, b = vs.alloc((1, 5)), vs.alloc((2, 4)), vs.alloc((0, 1))
    cs.alloc(M.Or((M.XEqY(x, y), M.Boolean(b))))
    bits = np.stack([bits_of([1, 3, 5]), bits_of([2, 4]), bits_of([0, 1])])[None]
    return vs, cs, bits


def hand_implication():
    """x = {2}, y = {1, 3}, z = {0..5}; one unit "x != y implies x < z".  The reference's implication(f, g) is Disjunction[f, g.not()]
    (logic/mod.rs:30-36): the CONCLUSION comes first, so the unit is implication(XLessY(x, z), XNeqY(x, y)) = Or(XLessY(x, z), XEqY(x, y))."""
    vs, cs = M.VStore(), M.CStore()
    x, y, z = vs.alloc((2, 2)), vs.alloc((1, 3)), vs.alloc((0, 5))
    cs.alloc(M.implication(M.XLessY(x, z), M.XNeqY(x, y)))
    bits = np.stack([bits_of([2]), bits_of([1, 3]), bits_of(range(6))])[None]
    return vs, cs, bits


def disjunctive_schedule(durations=(2, 3, 2, 1), horizon=8):
    """Four tasks on one machine: starts s_i in [0, horizon - d_i], pairwise Or(s_i + d_i <= s_j, s_j + d_j <= s_i), and
    equivalence(Boolean(b), XLessY(s_0, s_2)).  Returns (vs, cs, starts, b)."""
    vs, cs = M.VStore(), M.CStore()
    s = [vs.alloc((0, horizon - d)) for d in durations]
    b = vs.alloc((0, 1))
    for i in range(len(s)):
        for j in range(i + 1, len(s)):
            cs.alloc(M.Or((M.x_leq_y(M.Addition(s[i], durations[i]), s[j]), M.x_leq_y(M.Addition(s[j], durations[j]), s[i]))))
    cs.alloc(M.equivalence(M.Boolean(b), M.XLessY(s[0], s[2])))
    return vs, cs, s, b


@functools.lru_cache(maxsize=None)
def wide_case(seed, n_extra=60, n_nodes=24):
    """A random store of random_case's shape with `n_extra` more units, each a Disjunction of two or three random leaves over the same 12
    variables (weak enough that, for some seeds, many nodes survive 70 units: the callers name those seeds), and random set-valued nodes."""
    from util import splitmix64
    vs, cs = random_formula_store(seed)
    rng = splitmix64(seed + 7)
    n = len(vs)
    views = [M.Identity(i) for i in range(n)]

    def leaf():
        k = int(rng.integers(0, 4))
        a, b = (views[i] for i in rng.choice(n - 3, size=2, replace=False))
        off = int(rng.integers(-2, 3))
        if k == 3:
            bv = views[n - 3 + int(rng.integers(0, 3))]
            return M.Boolean(bv) if rng.random() < 0.5 else M.BooleanNeg(bv)
        return (M.XNeqY, M.XEqY, M.XLessY)[k](a, M.Addition(b, off))

    for _ in range(n_extra):
        cs.alloc(M.Or(tuple(leaf() for _ in range(int(rng.integers(2, 4))))))
    lb, ub = vs.bounds()
    bits = random_sets(seed + 1000, lb, ub, n_nodes, 1, 0, p_keep=0.8)
    bits.setflags(write=False)
    return vs, cs, bits
