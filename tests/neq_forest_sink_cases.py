"""What the tests of the all-XNeqY forest's solution sink share (test_neq_forest_sink_cpu.py, test_neq_forest_sink_gpu.py;
pcp_dfs_forest_device_neq_sink): four all-XNeqY models — N-queens 6 and 8 (the pinned sets of forest_sink_cases.py), a box model whose search
has True nodes wider than one point, a wide store of 601 variables —, for each a brute-force point set computed in plain Python from the
constraints themselves, and the checks a returned set of boxes must pass against it.  TEST INFRASTRUCTURE."""
import functools
import itertools

import numpy as np

import forest_sink_cases as K
from pcp_amd import model as M

CASES = ("queens6", "queens8", "box", "wide")
N_SOLUTIONS = {"queens6": K.N_SOLUTIONS["queens6"], "queens8": K.N_SOLUTIONS["queens8"], "box": 8, "wide": 2}

# The box model: a, c in [0, 1]; b in [5, 8]; d in [5, 6]; a != c; a != b (entailed at the root: the domains are disjoint); d != c + 5.
# Whatever a is, c and d follow and b stays free: each True node is a box of four points, and lower bounds alone would lose three of them.
BOX_DOMS = ((0, 1), (5, 8), (0, 1), (5, 6))
BOX_POINTS = frozenset({(0, 5, 1, 5), (0, 6, 1, 5), (0, 7, 1, 5), (0, 8, 1, 5), (1, 5, 0, 6), (1, 6, 0, 6), (1, 7, 0, 6), (1, 8, 0, 6)})

# The wide store: 4-queens in variables 0 .. 3; variables 4 .. 600 singletons with pairwise different values (100 + i), each tied to its
# predecessor and to one queen by XNeqY.  601 cells: more than a 512-thread workgroup has threads, and no multiple of 64.
WIDE_V = 601
WIDE_QUEENS = ((2, 4, 1, 3), (3, 1, 4, 2))


@functools.lru_cache(maxsize=None)
def build(name):
    """(vs, cs) of the model."""
    if name.startswith("queens"):
        return K.build(name)
    vs, cs = M.VStore(), M.CStore()
    if name == "box":
        a, b, c, d = (vs.alloc(dom) for dom in BOX_DOMS)
        cs.alloc(M.XNeqY(a, c))
        cs.alloc(M.XNeqY(a, b))
        cs.alloc(M.XNeqY(d, M.Addition(c, 5)))
        return vs, cs
    assert name == "wide"
    q = [vs.alloc((1, 4)) for _ in range(4)]
    for i in range(4):
        for j in range(i + 1, 4):
            cs.alloc(M.XNeqY(q[i], q[j]))
            cs.alloc(M.XNeqY(q[i], M.Addition(q[j], j - i)))
            cs.alloc(M.XNeqY(q[i], M.Addition(q[j], i - j)))
    xs = list(q)
    for i in range(4, WIDE_V):
        xs.append(vs.alloc((100 + i, 100 + i)))
        cs.alloc(M.XNeqY(xs[i], xs[i - 1]))
        cs.alloc(M.XNeqY(xs[i], xs[i % 4]))
    return vs, cs


def root(name):
    vs, _ = build(name)
    lb0, ub0 = vs.bounds()
    return np.ascontiguousarray(lb0, np.int32), np.ascontiguousarray(ub0, np.int32)


def hull(name):
    lb0, ub0 = root(name)
    return int(lb0.min()), int(ub0.max())


def push(ctx, name, declare_hull=False):
    """Push the model into a device context, with or without a declared hull; (lb0, ub0)."""
    vs, cs = build(name)
    M.push_model(ctx, cs, len(vs))
    if declare_hull:
        ctx.set_hull(*hull(name))
    return root(name)


@functools.lru_cache(maxsize=None)
def brute(name):
    """The model's solutions as a frozenset of full assignments, from the constraints themselves."""
    if name.startswith("queens"):
        return K.brute(name)
    if name == "box":
        out = set()
        for a, b, c, d in itertools.product(*[range(l, u + 1) for l, u in BOX_DOMS]):
            if a != c and a != b and d != c + 5:
                out.add((a, b, c, d))
        return frozenset(out)
    out = set()
    tail = tuple(100 + i for i in range(4, WIDE_V))
    for p in itertools.permutations(range(1, 5)):
        if all(abs(p[i] - p[j]) != j - i for i in range(4) for j in range(i + 1, 4)):
            full = tuple(p) + tail
            assert all(full[i] != full[i - 1] and full[i] != full[i % 4] for i in range(4, WIDE_V))
            out.add(full)
    return frozenset(out)


def check_boxes(name, lbs, ubs):
    """The boxes are non-empty and pairwise disjoint, every point of every box is a solution, and together they are the brute-force set.
    Returns the number of boxes wider than one point."""
    sols = brute(name)
    seen, proper = set(), 0
    lbs, ubs = np.asarray(lbs), np.asarray(ubs)
    assert lbs.shape == ubs.shape and lbs.ndim == 2 and lbs.shape[1] == len(root(name)[0])
    for k, (l, u) in enumerate(zip(lbs, ubs)):
        assert (l <= u).all(), (k, l, u)
        proper += int((l < u).any())
        for p in K.points(l, u):
            assert p in sols, (name, k, p[:8])
            assert p not in seen, (name, k, p[:8], "covered twice")
            seen.add(p)
    assert seen == sols, (name, len(seen), len(sols))
    return proper


def stand_in(name):
    """The oracle-backed stand-in of engine.Context over the model (the one the CPU tests of the small-store forests use)."""
    from test_small_excl_cpu import SmallExclOracleCtx
    vs, cs = build(name)
    return SmallExclOracleCtx(len(vs), cs.lower(len(vs)))
