"""What the tests of Enumerate in the formula-store forest share (test_form_enum_forest_cpu.py, test_form_enum_forest_gpu.py;
pcp_dfs_forest_device_form_enum): FormTreeSim — small_enum_forest_cases.TreeSim over a store WITH formula units, the judge of a node being
form_excl_cases.judge (the oracle on the store plus one XNeqY(x, Constant(v)) per entry) — the shifted schedules of the negative-domain
tests with a judge of their own, and the sweep roots over "wide".  TEST INFRASTRUCTURE."""
import functools

import numpy as np

import form_excl_cases as X
import form_forest_cases as FC
from oracle import oracle as orc
from pcp_amd import model as M
from pcp_amd import search as S
from small_enum_forest_cases import NONE, counts, inside  # noqa: F401
from small_excl_cases import units

SEARCH_NAMES = ("A4", "C4mk", "D5mk")
# Without an objective the five-task model's Enumerate tree is far beyond form_excl_cases.TREE_CEILING (MiddleVal: 284 679 nodes — minutes of
# oracle calls, and of one wavefront): the tests walk its first WALK_LIMIT nodes under StopNode, on the specification and on the device
# alike.  Under its objective (the makespan minimised) the tree is some 5 000 nodes and is walked whole.
WALK_LIMIT = {"D5mk": 6000}
# (nodes, solutions, failed) of its COMPLETE trees: search.dfs_enumerate over test_form_excl_cpu.FormExclOracleCtx, computed once (four
# minutes of oracle calls each) and pinned; the suite re-derives the first WALK_LIMIT nodes only
D5MK_COMPLETE = {"middle": (284679, 24089, 118251), "min": (159513, 23559, 56198)}


# ---------------------------------------------------------------------------------------------------------------- stores and judges
@functools.lru_cache(maxsize=None)
def shifted(name, shift):
    """(vs, cs, mk, lb0, ub0) of form_forest_cases.schedule(name, shift): start windows that reach below zero."""
    vs, cs, mk = FC.schedule(name, shift)
    lb0, ub0 = vs.bounds()
    return vs, cs, mk, np.ascontiguousarray(lb0, np.int32), np.ascontiguousarray(ub0, np.int32)


_SHIFTED, _JUDGED = {}, {}


def judge(key, L, U, ex):
    """(status, lb, ub) of one node: ``key`` a store name of form_excl_cases (its judge), or (name, shift) — the oracle on that shifted
    schedule plus one XNeqY per entry, computed once per distinct node."""
    if isinstance(key, str):
        return X.judge(key, L, U, ex)
    ex = tuple((int(a), int(b)) for a, b in ex)
    k = (key, L.tobytes(), U.tobytes(), ex)
    if k not in _JUDGED:
        if (key, ex) not in _SHIFTED:
            vs, cs, *_ = shifted(*key)
            om = orc.OracleModel(len(vs))
            M.push_model(om, cs, len(vs))
            if ex:
                om.push_props(units(ex))
            if len(_SHIFTED) > 4096:
                _SHIFTED.clear()
            _SHIFTED[(key, ex)] = om
        r = _SHIFTED[(key, ex)].consistency(L[None], U[None], None)
        _JUDGED[k] = (int(r[3][0]), r[0][0].copy(), r[1][0].copy())
    return _JUDGED[k]


def root_of(key):
    """(lb0, ub0) of a store."""
    if isinstance(key, str):
        _, _, _, lb0, ub0, _, _ = X.store(key)
    else:
        _, _, _, lb0, ub0 = shifted(*key)
    return np.ascontiguousarray(lb0, np.int32), np.ascontiguousarray(ub0, np.int32)


# ---------------------------------------------------------------------------------------------------------------- one tree
class FormTreeSim:
    """One tree of the Enumerate forest over a formula store: rows[r] = (lb, ub), row_base[r], row_excl[r] (None or (var, value)) for r in
    [0, sp), and `path` — small_enum_forest_cases.TreeSim, the judge of a node being judge() above on the entries of the path that lie inside
    the node's domains (the others are entailed).  ``node_limit``: StopNode's, as the kernel keeps it.  step() does what one kernel step does
    and leaves what a launch that ends there leaves."""

    def __init__(self, key, val="middle", objective=None, root=None, root_excl=(), node_limit=0):
        self.key, self.node_limit, self.stopped = key, node_limit, False
        lb0, ub0 = root_of(key) if root is None else (np.ascontiguousarray(root[0], np.int32), np.ascontiguousarray(root[1], np.int32))
        self.val, self.obj = val, objective
        self.path = [(int(x), int(v)) for x, v in root_excl]
        self.rows, self.row_base, self.row_excl = [(lb0.copy(), ub0.copy())], [len(self.path)], [None]
        self.nodes = self.solutions = self.failed = 0
        self.best, self.best_row, self.incumbents = None, None, []
        self.rechosen = 0      # nodes at which the selector's value was excluded already and another one was taken
        self.max_path = len(self.path)
        self.last = None       # of the last step: (lb_in, ub_in, list, status, lb_out, ub_out)
        self.boxes = []        # the Satisfiable nodes as (lb, ub)

    @property
    def sp(self):
        return len(self.rows)

    def top(self):
        """(lb, ub, row_base, (var, value) or (NONE, 0), path[:row_base]) of the top row."""
        r = self.sp - 1
        e = self.row_excl[r]
        return self.rows[r][0], self.rows[r][1], self.row_base[r], (e if e is not None else (NONE, 0)), list(self.path[:self.row_base[r]])

    def step(self):
        r = self.sp - 1
        L, U = (a.copy() for a in self.rows[r])
        n = self.row_base[r]
        del self.path[n:]
        if self.row_excl[r] is not None:
            self.path.append(self.row_excl[r])
            n += 1
        self.max_path = max(self.max_path, n)
        self.rows.pop(); self.row_base.pop(); self.row_excl.pop()
        self.nodes += 1
        if self.obj is not None and self.best is not None:  # the bound, folded as the row is popped
            var, mode = self.obj
            if mode == "min":
                U[var] = min(U[var], self.best - 1)
            else:
                L[var] = max(L[var], self.best + 1)
            if L[var] > U[var]:
                self.failed += 1
                self.last = (L, U, list(self.path), 0, L, U)
                return
        ex = np.array(self.path, np.int32).reshape(-1, 2)
        status, lb, ub = judge(self.key, L, U, [e for e in self.path if L[e[0]] <= e[1] <= U[e[0]]])
        self.last = (L, U, list(self.path), status, lb, ub)
        # StopNode: the node that reaches the limit is a node, but neither a solution nor a failure; it is still branched on
        last = bool(self.node_limit) and self.nodes >= self.node_limit
        self.stopped |= last
        if last and status != 2:
            pass
        elif status == 0:
            self.failed += 1
        elif status == 1:
            self.solutions += 1
            self.boxes.append((lb.copy(), ub.copy()))
            if self.obj is not None:
                self.best, self.best_row = int(lb[self.obj[0]]), lb.copy()
                self.incumbents.append(self.best)
        else:
            cl, cu, _, _, dirty = S.branch_enumerate(lb, ub, [0, len(ex)], ex, val=self.val)
            x = int(dirty[0])
            v = int(cl[0, x])
            m = int(S.middle_val(lb[x:x + 1], ub[x:x + 1])[0]) if self.val == "middle" else int(lb[x])
            self.rechosen += v != m
            folded = v == lb[x] or v == ub[x]
            # the parent's row becomes the right child, the left child goes on top with the path as it is
            self.rows += [(cl[1].copy(), cu[1].copy()), (cl[0].copy(), cu[0].copy())]
            self.row_base += [n, n]
            self.row_excl += [None if folded else (x, v), None]

    def run(self, on_node=None, limit=1 << 30):
        while self.sp and not self.stopped and self.nodes < limit:
            self.step()
            if on_node:
                on_node(self)
        return self.nodes, self.solutions, self.failed


@functools.lru_cache(maxsize=None)
def tree(key, val, objective=None):
    """The complete tree of a store's root, once: the finished FormTreeSim."""
    sim = FormTreeSim(key, val, objective=objective)
    sim.run()
    return sim


# ---------------------------------------------------------------------------------------------------------------- the sweep's lane stride
SWEEP_SIZES = (63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def sweep_roots():
    """[(lb0, ub0, list)] over "wide": lists of 63, 64, 65 and 130 entries — interior values, a few outside the domain, one at each bound of a
    start — then the lists of form_excl_cases.chain_cases() (the last: 70 consecutive values from a bound, 70 rounds)."""
    lb0, ub0 = root_of("wide")
    rng = np.random.default_rng(7311)
    out = []
    for c in SWEEP_SIZES:
        xs = rng.integers(0, 4, c)
        vals = rng.integers(2, 99, c)           # interior
        vals[:3] = (-5, 101, 250)               # outside the domain
        vals[3], vals[4] = 0, 100               # one at each bound
        xs[3], xs[4] = 1, 2
        ex = [(int(a), int(b)) for a, b in zip(xs, vals)]
        rng.shuffle(ex)
        out.append((lb0, ub0, [tuple(e) for e in ex]))
    _, L, U, excl, chain = X.chain_cases()
    assert len(excl[chain]) == X.CHAIN
    for i in range(len(excl)):
        out.append((np.ascontiguousarray(L[i], np.int32), np.ascontiguousarray(U[i], np.int32), [tuple(e) for e in excl[i]]))
    return out
