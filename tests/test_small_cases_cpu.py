"""The cases of small_cases.py, specification side (no GPU): the oracle's answers on them reach the edges of smallfix_kernel
(pcp_small.hip) that each case is named for, so that test_small_edges_gpu.py cannot pass on inputs that miss them.  Every case carries
its own predicates over the oracle's result (`expect`); the ones the lowering decides — slot and unit counts, which Distinct units
enter the all-different table — are computed from the rows by small_cases.slot_count / alldiff_units, which restate lower_model and
lower_alldiff (pcp_lower.hip; tests/lower_check.cpp pins those against hand-written tables)."""
import numpy as np
import pytest

from oracle import oracle as orc
from pcp_amd import model as M

import small_cases as SC


def check(case, ref):
    name, n_vars, props, L, U, act, expect = case
    st = ref[3]
    print(name, "V", n_vars, "S", SC.slot_count(props, n_vars), "P", len(props), "nodes", len(L), "False/True/Unknown", np.bincount(st, minlength=3).tolist())
    assert L.shape == U.shape == (len(st), n_vars) and np.abs(L).max() <= 1000 and np.abs(U).max() <= 1000
    for what, pred in expect.items():
        assert pred(ref), f"{name}: {what}"


@pytest.mark.parametrize("key", SC.CASES)
def test_case_reaches_its_edge(key):
    check(SC.CASES[key](), SC.reference(key))


def test_the_restated_lowering_on_the_checker_s_own_tables():
    """small_cases.alldiff_units on the tables of lower_check.cpp's "all-different detection": one unit of four variables behind a
    standalone record; a missing pair, an offset; nine units of three variables, of which the table keeps eight."""
    def distinct(vs, first):
        return M.lower_units([M.Distinct([M.Identity(v) for v in vs])], 32, gid_base=first)
    one = np.concatenate([M.lower_units([M.XNeqY(M.Identity(4), M.Identity(5))], 6), distinct([0, 1, 2, 3], 1)])
    assert SC.alldiff_units(one, 6) == ([(1, [0, 1, 2, 3])], []) and SC.unit_of_prop(one).tolist() == [0] + [1] * 6
    assert SC.alldiff_units(one[:-1], 6) == ([], [])
    off = one.copy(); off["off"][3][1] = 1
    assert SC.alldiff_units(off, 6) == ([], [])
    nine = np.concatenate([distinct([3 * u, 3 * u + 1, 3 * u + 2], u) for u in range(9)])
    grouped, left = SC.alldiff_units(nine, 27)
    assert grouped == [(u, [3 * u, 3 * u + 1, 3 * u + 2]) for u in range(8)] and left == [(8, [24, 25, 26])]
    consts = M.lower_units([M.XLessY(M.Identity(0), M.Constant(5)), M.XNeqY(M.Identity(1), M.Constant(5)), M.XLessY(M.Constant(-5), M.Identity(2))], 3)
    assert SC.slot_count(consts, 3) == 5


def test_the_shapes_cover_the_staging_edges():
    assert {SC.slot_count(*SC.CASES[f"B-S{s}"]()[2:0:-1]) for s in SC.B_SLOTS} == {63, 64, 65, 127, 128}
    units = {orc.OracleModel(*SC.CASES[f"B-U{u}"]()[1:3]).n_units for u in SC.B_UNITS}
    assert units == {1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 129}
    assert {(u + 31) // 32 for u in units} == {1, 2, 3, 4, 5} and {(u + 63) // 64 for u in units} == {1, 2, 3}
    for key in SC.LIMIT_CASES:  # beyond the path's limits in ONE of the two figures
        _, n_vars, props, _, _, _, _ = SC.CASES[key]()
        assert (SC.slot_count(props, n_vars), len(props) <= 2048) == (129, True) or (SC.slot_count(props, n_vars) <= 128, len(props)) == (True, 2049)
    for key in SC.CASES:
        if key not in SC.LIMIT_CASES:
            _, n_vars, props, _, _, _, _ = SC.CASES[key]()
            assert SC.slot_count(props, n_vars) <= 128 and len(props) <= 2048, key
    assert SC.C_NODES > 8 * 256 * 4 and SC.C_NODES % SC.C_PERIOD != 0
    assert set(SC.DISTINCT_CASES) | {"C"} == {k for k in SC.CASES if SC.alldiff_units(*SC.CASES[k]()[2:0:-1])[0]}


def test_node_units_case():
    case, units = SC.d_case()
    assert len(units) == len(case[3]) and max(len(u) for u in units) == 70
    check(case, SC.d_reference())
