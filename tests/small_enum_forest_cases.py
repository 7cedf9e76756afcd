"""What the tests of Enumerate in the small-store forest share (test_small_enum_forest_cpu.py, test_small_enum_forest_gpu.py;
pcp_dfs_forest_device_small_enum): the models of small_forest_cases.py as (n_vars, props, lb0, ub0), the oracle-backed stand-in context
the host specification search.dfs_enumerate runs on, and TreeSim — a numpy restatement of ONE tree's state as the kernel keeps it between
launches: the stack rows, row_base, row_excl and the exclusion path, stepped node by node with search.branch_enumerate's value rule and
the oracle as the judge of a node.  TEST INFRASTRUCTURE."""
import functools

import numpy as np

import small_excl_cases as X
import small_forest_cases as C
from pcp_amd import search as S

NONE = 0xFFFFFFFF  # row_excl[r].var of a row that appends nothing


@functools.lru_cache(maxsize=None)
def model(name):
    """(n_vars, lowered props, lb0, ub0, objective variable or None) of "golomb5" / "golomb6" / "queens8" / "golomb5-3" / a STORES name."""
    var = None
    if name.startswith("golomb") and "-" not in name:
        vs, cs, var = C.golomb(int(name[6:]))
    elif name == "golomb5-3":
        vs, cs = C.golomb_shifted(5, -3)
    elif name == "queens8":
        vs, cs = C.queens8()
    else:
        vs, cs = C.store(name)
    lb0, ub0 = vs.bounds()
    return len(vs), cs.lower(len(vs)), np.ascontiguousarray(lb0, np.int32), np.ascontiguousarray(ub0, np.int32), var


def stand_in(name):
    """The oracle-backed context of the Enumerate CPU tests over that model."""
    from test_small_excl_cpu import SmallExclOracleCtx
    V, props, *_ = model(name)
    return SmallExclOracleCtx(V, props)


def counts(st):
    return st.num_nodes, st.num_solution, st.num_failed_node


def inside(entries, lb, ub):
    """The entries whose value lies inside their variable's domain, as a set of (var, value)."""
    return {(int(x), int(v)) for x, v in entries if lb[int(x)] <= int(v) <= ub[int(x)]}


class TreeSim:
    """One tree of the Enumerate forest: rows[r] = (lb, ub), row_base[r], row_excl[r] (None or (var, value)) for r in [0, sp), and `path`.
    Node r is the row's bounds under path[:row_base[r]] plus row_excl[r].  step() does what one kernel step does and leaves what a launch
    that ends there leaves: a left child nobody has popped is a row with row_base = n and no entry."""

    def __init__(self, name, val="middle", objective=None, root=None, root_excl=()):
        self.V, self.props, lb0, ub0, _ = model(name)
        lb0, ub0 = (lb0, ub0) if root is None else (np.ascontiguousarray(root[0], np.int32), np.ascontiguousarray(root[1], np.int32))
        self.val, self.obj = val, objective
        self.path = [(int(x), int(v)) for x, v in root_excl]
        self.rows, self.row_base, self.row_excl = [(lb0.copy(), ub0.copy())], [len(self.path)], [None]
        self.nodes = self.solutions = self.failed = 0
        self.best, self.best_row = None, None
        self.rechosen = 0      # nodes at which the selector's value was excluded already and another one was taken
        self.max_path = len(self.path)
        self.last = None       # of the last step: (lb_in, ub_in, list, status)

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
                self.last = (L, U, list(self.path), 0)
                return
        ex = np.array(self.path, np.int32).reshape(-1, 2)
        status, lb, ub = X.judge(self.V, self.props, L, U, [e for e in self.path if L[e[0]] <= e[1] <= U[e[0]]])
        self.last = (L, U, list(self.path), status)
        if status == 0:
            self.failed += 1
        elif status == 1:
            self.solutions += 1
            if self.obj is not None:
                self.best, self.best_row = int(lb[self.obj[0]]), lb.copy()
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

    def run(self, on_node=None):
        while self.sp:
            self.step()
            if on_node:
                on_node(self)
        return self.nodes, self.solutions, self.failed
