"""What the tests of Enumerate in the all-XNeqY forest share (test_neq_enum_forest_cpu.py, test_neq_enum_forest_gpu.py;
pcp_dfs_forest_device_neq_enum): N-queens models as (n_vars, props, lb0, ub0), the oracle-backed stand-in context the host specification
search.dfs_enumerate runs on, and TreeSim (small_enum_forest_cases.py) over them — the numpy restatement of ONE tree's rows, row_base,
row_excl and exclusion path between launches.  TEST INFRASTRUCTURE."""
import functools

import numpy as np

import small_enum_forest_cases as EC
from pcp_amd import model as M

NONE = EC.NONE
SIZES = (4, 5, 6, 8)                       # the one-tree cases of the GPU tests
SOLUTIONS = {4: 2, 5: 10, 6: 4, 8: 92}     # N-queens solution counts


@functools.lru_cache(maxsize=None)
def queens(n):
    """(n_vars, lowered props, lb0, ub0) of model.nqueens(n) — queens8 is small_forest_cases.queens8's store."""
    vs, cs = M.nqueens(n)
    lb0, ub0 = vs.bounds()
    return len(vs), cs.lower(len(vs)), np.ascontiguousarray(lb0, np.int32), np.ascontiguousarray(ub0, np.int32)


def stand_in(n):
    """The oracle-backed context of the Enumerate CPU tests over N-queens-n."""
    from test_small_excl_cpu import SmallExclOracleCtx
    V, props, _, _ = queens(n)
    return SmallExclOracleCtx(V, props)


def push(ctx, n):
    """Push N-queens-n into a device context; (lb0, ub0)."""
    vs, cs = M.nqueens(n)
    M.push_model(ctx, cs, len(vs))
    return queens(n)[2], queens(n)[3]


class TreeSim(EC.TreeSim):
    """small_enum_forest_cases.TreeSim over N-queens-n: the same steps, the model taken from queens(n)."""

    def __init__(self, n, val="middle", root=None, root_excl=()):
        self.V, self.props, lb0, ub0 = queens(n)
        lb0, ub0 = (lb0, ub0) if root is None else (np.ascontiguousarray(root[0], np.int32), np.ascontiguousarray(root[1], np.int32))
        self.val, self.obj = val, None
        self.path = [(int(x), int(v)) for x, v in root_excl]
        self.rows, self.row_base, self.row_excl = [(lb0.copy(), ub0.copy())], [len(self.path)], [None]
        self.nodes = self.solutions = self.failed = 0
        self.best, self.best_row = None, None
        self.rechosen = 0
        self.max_path = len(self.path)
        self.last = None


def is_queens(row, n):
    """row[:n] places n queens that do not attack each other (columns 1 .. n, one per row)."""
    q = [int(x) for x in row[:n]]
    return (sorted(q) == list(range(1, n + 1)) and len({q[i] + i for i in range(n)}) == n and len({q[i] - i for i in range(n)}) == n)
