"""The reference figures of the formula-store forest tests (test_setform_forest_gpu.py), without a GPU: the restatement of the search
loop in setform_forest_ref.py against the oracle's own DFS over FDSpace under BinarySplit, and the counts it and
test_bnb_forest_cpu.reference_bnb_set_any give on the schedule models, pinned."""
import numpy as np
import pytest

import setform_cases as SC
import setform_forest_ref as R

# (durations, horizon, makespan variable) -> nodes / solutions / failed under BinarySplit
SPLIT = {
    (R.DUR4, 8, False): (61, 24, 7),
    (R.DUR4, 8, True): (73, 24, 13),
    (R.DUR4, 11, False): (997, 490, 9),
    (R.DUR5, 16, False): (3217, 1584, 25),
}


@pytest.mark.parametrize("durations,horizon,makespan", list(SPLIT))
def test_the_restatement_under_binary_split_is_the_oracles_search(durations, horizon, makespan):
    vs, cs, _ = R.schedule(durations, horizon, makespan)
    lb0, ub0 = vs.bounds()
    ss = SC.oracle_model(vs, cs).search_set(lb0, ub0, 1, 0, all_solutions=True)[0]
    got = R.schedule_counts(durations, horizon, makespan)
    assert got == (ss["num_nodes"], ss["num_solution"], ss["num_failed_node"]) == SPLIT[(durations, horizon, makespan)]


def test_the_restatement_at_a_node_limit_is_the_oracles_search():
    """StopNode: the node that reaches the limit is counted, but is neither a solution nor a failure."""
    vs, cs, _ = R.schedule(R.DUR4, 8, False)
    lb0, ub0 = vs.bounds()
    ss = SC.oracle_model(vs, cs).search_set(lb0, ub0, 1, 0, all_solutions=True, node_limit=20)[0]
    assert R.schedule_counts(R.DUR4, 8, False, node_limit=20) == (ss["num_nodes"], ss["num_solution"], ss["num_failed_node"]) == (20, 6, 3)
    assert R.schedule_counts(R.DUR4, 8, False, "enumerate", "middle", 20) == (20, 2, 6)
    assert R.schedule_counts(R.DUR4, 8, False, "enumerate", "min", 20) == (20, 4, 4)


def test_every_solution_of_the_restatement_is_a_schedule():
    vs, cs, _ = R.schedule(R.DUR4, 8, False)
    for brancher, val in R.BRANCHERS:
        r = R.reference_search(SC.oracle_model(vs, cs), SC.hull_sets(vs, 1, 0), 0, brancher, val)
        assert r["solutions"] == len(r["rows"]) == 24 and all(R.schedule_is_valid(row) for row in r["rows"])


def test_the_word_boundary_changes_nothing():
    """set_words = 2 from -60: the domains 0..7 straddle words 0 and 1; the counts are the one-word ones under every distributor."""
    vs, _, _ = R.schedule(R.DUR4, 8, False)
    bits = SC.hull_sets(vs, 2, -60)
    assert (bits[:4, 0] >> np.uint64(60)).all() and (bits[:4, 1] & np.uint64(1)).all()
    for brancher, val in R.BRANCHERS:
        assert R.schedule_counts(R.DUR4, 8, False, brancher, val, 0, 2, -60) == R.schedule_counts(R.DUR4, 8, False, brancher, val)


def test_minimising_the_makespan():
    """nodes / failed / solutions, best and incumbents of reference_bnb_set_any on the two makespan models."""
    want = {
        (R.DUR4, 8, "split", "middle"): (29, 14, 1, 8, [8]),
        (R.DUR4, 8, "enumerate", "middle"): (55, 27, 1, 8, [8]),
        (R.DUR4, 8, "enumerate", "min"): (31, 15, 1, 8, [8]),
        (R.DUR5, 16, "split", "middle"): (193, 96, 1, 14, [14]),
        (R.DUR5, 16, "enumerate", "middle"): (425, 210, 3, 14, [16, 15, 14]),
        (R.DUR5, 16, "enumerate", "min"): (213, 106, 1, 14, [14]),
    }
    for (durations, horizon, brancher, val), figures in want.items():
        r = R.schedule_bnb(durations, horizon, brancher, val)
        assert (r["nodes"], r["failed"], r["solutions"], r["best"], r["incumbents"]) == figures
        assert R.schedule_is_valid(r["row"], durations, makespan=r["best"]) and int(r["row"][-1]) == r["best"]


def test_random_formula_stores_from_the_hull():
    """The seeds the device test searches: 6 and 8 finish below 2000 nodes, 4, 7 and 9 reach the limit with solutions and failures, 0 fails
    at the root; the restatement at the limit is the oracle's search."""
    want = {0: (1, 0, 1), 6: (313, 86, 71), 8: (369, 161, 24)}
    for seed in (0, 4, 6, 7, 8, 9):
        vs, cs, _ = SC.random_case(seed)
        om = SC.oracle_model(vs, cs)
        lb0, ub0 = vs.bounds()
        ss = om.search_set(lb0, ub0, 1, 0, all_solutions=True, node_limit=2000)[0]
        got = (ss["num_nodes"], ss["num_solution"], ss["num_failed_node"])
        r = R.reference_search(om, SC.hull_sets(vs, 1, 0), 0, node_limit=2000)
        assert (r["nodes"], r["solutions"], r["failed"]) == got
        if seed in want:
            assert got == want[seed]
        else:
            assert got[0] == 2000 and got[1] > 0 and got[2] > 0


def test_the_library_exports_the_forest_entries_for_formula_stores():
    import pcp_amd.engine as E
    import pcp_amd.search_forest as SF
    import inspect
    import test_abi
    L = test_abi._built()
    for name in ("pcp_dfs_forest_device_setform", "pcp_dfs_forest_device_setform_bnb"):
        assert name in E.ABI_SYMBOLS and hasattr(L, name)
    assert callable(E.Context.dfs_forest_setform) and callable(E.Context.dfs_forest_setform_bnb)
    for f in (SF.forest_search_set, SF.forest_bnb_set):
        assert inspect.signature(f).parameters["formulas"].default is False
