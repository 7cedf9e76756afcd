"""The reified layer over IntervalSet stores, specification side (no GPU): hand-derived vectors through the oracle's IntervalSet
instantiation (oracle/pcp_oracle_engine.inc, namespace orc::fdset), the share of the random generator the GPU parity tests
(test_setform_gpu.py) draw from, and the lowering of formula units in set mode (tests/lower_setform_check.cpp, a program of its own
under AddressSanitizer and UBSan)."""
import os
import subprocess

import numpy as np

from pcp_amd import model as M

import setform_cases as SC
from test_set_mode import values_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def interval_mode(om, bits, base):
    """Interval-mode propagation of the same nodes' bounds: (lb, ub, status)."""
    lb, ub = M.bits_bounds(bits, base)
    r = om.consistency(lb.astype(np.int32), ub.astype(np.int32), None)
    return r[0], r[1], r[3]


def test_disjoint_sets_disentail_xeqy_and_the_disjunction_propagates_boolean():
    """x = {1, 3, 5}, y = {2, 4}: XEqY is False over sets (disjoint, although the hulls overlap), so Or(XEqY(x, y), Boolean(b)) propagates
    Boolean: b = {1}, the unit is entailed, status True.  Over the intervals [1, 5], [2, 4] XEqY is Unknown and nothing moves."""
    vs, cs, bits = SC.hand_or_eq_bool()
    om = SC.oracle_model(vs, cs)
    lb, ub, out, act, st, _ = om.consistency_set(bits, 0)
    assert st[0] == M.TRUE and int(act[0, 0]) == 0
    assert [values_of(w) for w in out[0]] == [[1, 3, 5], [2, 4], [1]]
    assert (lb[0].tolist(), ub[0].tolist()) == ([1, 2, 1], [5, 4, 1])
    li, ui, sti = interval_mode(om, bits, 0)
    assert sti[0] == M.UNKNOWN and (li[0].tolist(), ui[0].tolist()) == ([1, 2, 0], [5, 4, 1])


def test_premise_entailed_over_sets_only():
    """x = {2}, y = {1, 3}: x != y is True over sets and Unknown over [1, 3]; "x != y implies x < z" takes 0..2 from z in set mode only."""
    vs, cs, bits = SC.hand_implication()
    om = SC.oracle_model(vs, cs)
    lb, ub, out, act, st, _ = om.consistency_set(bits, 0)
    assert [values_of(w) for w in out[0]] == [[2], [1, 3], [3, 4, 5]]
    assert st[0] == M.TRUE and int(act[0, 0]) == 0  # x < z is entailed now: 2 < 3
    li, ui, sti = interval_mode(om, bits, 0)
    assert sti[0] == M.UNKNOWN and (li[0].tolist(), ui[0].tolist()) == ([2, 1, 0], [2, 3, 5])


def test_generator_covers_failures_open_nodes_and_set_only_behaviour():
    """The 40 random stores x 8 random nodes of the GPU parity tests: at least a quarter of the nodes fail, at least a quarter stay Unknown,
    and at least 20 differ from interval-mode propagation of their bounds (status, or the bounds of a node that did not fail)."""
    n_false = n_unknown = n_differ = total = 0
    for seed in SC.SEEDS:
        vs, cs, bits = SC.random_case(seed)
        assert len(vs) == 12
        lb, ub, _, _, st = SC.random_reference(seed)
        li, ui, sti = interval_mode(SC.oracle_model(vs, cs), bits, 0)
        total += len(st)
        n_false += int((st == M.FALSE).sum())
        n_unknown += int((st == M.UNKNOWN).sum())
        ok = (st != M.FALSE) & (sti != M.FALSE)
        n_differ += int(((st != sti) | (ok & ((lb != li).any(axis=1) | (ub != ui).any(axis=1)))).sum())
    print(f"set-mode formula generator: {n_false} False, {n_unknown} Unknown, {n_differ} differ from interval mode, of {total}")
    assert total == 320
    assert 4 * n_false >= total and 4 * n_unknown >= total and n_differ >= 20


def test_lowering_of_formulas_in_set_mode():
    exe = os.path.join(ROOT, "tests", "lower_setform_check")
    subprocess.run(["g++", "-x", "c++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                    "-o", exe, "tests/lower_setform_check.cpp", "pcp_amd/csrc/pcp_lower.hip"], cwd=ROOT, check=True)
    r = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr  # (a sanitizer report)
    assert r.stdout.splitlines() == ["ok formula tables in set mode", "ok set-mode refusals", "all ok"]
