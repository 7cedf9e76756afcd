"""The schedule models of the Interval formula forest tests (test_form_forest_cpu.py, test_form_forest_gpu.py): tasks under
propagators::Cumulative (Constant durations and resources, a capacity variable fixed to 3), optionally with a makespan variable — and the
oracle-backed stand-in of engine.Context that runs the host specification (pcp_amd.search.dfs) on them.  TEST INFRASTRUCTURE."""
import numpy as np

from oracle import oracle as orc
from pcp_amd import model as M

from oracle_ctx import OracleCtx

# name -> (durations, resources, start window, makespan window or None)
MODELS = {
    "A4": ((3, 2, 2, 1), (2, 1, 2, 1), (0, 5), None),
    "C4mk": ((3, 2, 2, 1), (2, 1, 2, 1), (0, 6), (0, 12)),
    "D5mk": ((3, 2, 4, 1, 2), (2, 1, 2, 1, 1), (0, 8), (0, 14)),
    "B5": ((3, 2, 2, 1, 2), (2, 1, 2, 1, 1), (0, 7), None),
    "six": ((3, 2, 2, 1, 2, 1), (2, 1, 2, 1, 1, 2), (0, 7), None),
}
CAPACITY = 3


def schedule(name, shift=0):
    """(vs, cs, index of the makespan variable or None); ``shift`` moves the start windows."""
    durations, resources, win, mk_win = MODELS[name]
    vs, cs = M.VStore(), M.CStore()
    starts = [vs.alloc((win[0] + shift, win[1] + shift)) for _ in durations]
    mk = vs.alloc(mk_win) if mk_win else None
    cap = vs.alloc((CAPACITY, CAPACITY))
    M.Cumulative(starts, [M.Constant(d) for d in durations], [M.Constant(r) for r in resources], cap).join(vs, cs)
    if mk is not None:
        for s, d in zip(starts, durations):
            cs.alloc(M.x_leq_y(M.Addition(s, d), mk))
    return vs, cs, (mk.idx if mk is not None else None)


def oracle_model(vs, cs):
    om = orc.OracleModel(len(vs))
    M.push_model(om, cs, len(vs))
    return om


class FormulaOracleCtx(OracleCtx):
    """OracleCtx over a store pushed unit by unit (formula units included)."""

    def __init__(self, vs, cs):
        self._m = oracle_model(vs, cs)
        self.n_vars = len(vs)
        self.n_units = self._m.n_units
        self.words = self._m.words


def is_schedule(name, row, shift=0):
    """The start times row[:n] respect the capacity at every instant (and the makespan variable, if any, covers every task)."""
    durations, resources, win, mk_win = MODELS[name]
    n = len(durations)
    s = [int(x) for x in row[:n]]
    for t in range(win[0] + shift, win[1] + shift + max(durations) + 1):
        if sum(r for si, d, r in zip(s, durations, resources) if si <= t < si + d) > CAPACITY:
            return False
    return mk_win is None or all(si + d <= int(row[n]) for si, d in zip(s, durations))


def counts(r):
    """(nodes, solutions, failed) of an oracle search dict, a SearchStats or a forest result dict."""
    if isinstance(r, dict):
        if "num_nodes" in r:
            return r["num_nodes"], r["num_solution"], r["num_failed_node"]
        return r["nodes"], r["solutions"], r["failed"]
    return r.num_nodes, r.num_solution, r.num_failed_node


def np_rows(*rows):
    return tuple(np.ascontiguousarray(r, np.int32) for r in rows)
