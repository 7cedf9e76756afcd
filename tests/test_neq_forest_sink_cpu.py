"""The solution sink of the all-XNeqY forest (pcp_dfs_forest_device_neq_sink), without a GPU: the header declares the entry, the built
library exports it, engine binds it and the Rust bindings mirror it; Context.dfs_forest_neq_solutions and search_forest.forest_solutions
refuse what they do not do before anything runs, and the refusals of the functions that were there before still stand; the constants of
neq_forest_sink_cases.py are pinned against brute force and the oracle — among them that the box model's search has True nodes wider
than one point, the reason a row of the sink is a box."""
import inspect
import os
import re

import numpy as np
import pytest

import forest_sink_cases as K
import neq_forest_sink_cases as NK
from pcp_amd import search as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pcp_dfs_forest_device_neq_sink"


def params(header, name):
    m = re.search(r"\bint32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, name
    return re.findall(r"[A-Za-z_0-9]+|\*|,", m.group(1))


def test_the_entry_is_declared_exported_and_bound():
    """Fails without the feature: nothing names the entry."""
    import ctypes as C
    import pcp_amd.engine as E
    import test_abi
    with open(os.path.join(ROOT, "include", "pcp_hip.h")) as f:
        header = f.read()
    # the parameter list of _neq_enum with the sink in the objective's place
    want = params(header, "pcp_dfs_forest_device_neq_enum")
    i = want.index("pcp_forest_objective")
    want[i], want[i + 2] = "pcp_solution_sink", "sink"
    assert params(header, NAME) == want
    assert re.search(r"#define\s+PCP_ABI_VERSION\s+8\b", header)
    doc = header[:header.index("int32_t " + NAME)]
    doc = doc[doc.rindex("/* Every solution of the all-XNeqY forest"):]
    assert "search/engine/all_solution.rs" in doc and "stop_node.rs:57-62" in doc
    assert NAME in E.ABI_SYMBOLS and hasattr(test_abi._built(), NAME)
    L = E.load_library()
    vp, u32 = C.c_void_p, C.c_uint32
    assert getattr(L, NAME).argtypes == [vp, C.POINTER(E.DfsState), u32, C.POINTER(E.ForestExcl), C.POINTER(E.PcpSolutionSink), u32, u32, C.c_uint64, vp]
    assert getattr(L, NAME).restype == C.c_int32
    with open(os.path.join(ROOT, "integration", "pcp-hip-sys", "src", "lib.rs")) as f:
        rust = f.read()
    sig = re.sub(r"\s+", " ", re.search(r"pub fn " + NAME + r"\(([^;]*)\) -> i32;", rust).group(1))
    assert sig == ("ctx: *mut pcp_ctx, st: *const pcp_dfs_state, n_trees: u32, ex: *const pcp_forest_excl, sink: *const pcp_solution_sink, "
                   "n_steps: u32, stop_on_solution: u32, node_limit: u64, hip_stream: *mut c_void")


def test_the_drivers_exist_with_the_documented_keywords():
    import pcp_amd.engine as E
    import pcp_amd.search_forest as SF
    p = inspect.signature(E.Context.dfs_forest_neq_solutions).parameters
    assert (p["brancher"].default, p["val"].default, p["root_excl"].default, p["sink_capacity"].default) == ("split", "middle", None, 4096)
    loop = ("stop_on_solution", "node_limit_per_tree", "steps_per_launch", "capacity", "max_launches", "node_budget", "want_solution", "rebalance", "info", "max_capacity",
            "hints", "path_capacity", "max_path")
    ref = inspect.signature(E.Context.dfs_forest).parameters
    assert all(p[k].default == ref[k].default for k in loop)
    q = inspect.signature(SF.forest_solutions).parameters
    assert (q["brancher"].default, q["val"].default, q["forest"].default, q["sink_capacity"].default) == ("split", "middle", None, 4096) and "n_trees" in q


class NotNeq:
    """A context whose store is not all-XNeqY: forest_solutions(forest="neq") must refuse it without touching anything else."""
    has_formulas, all_neq, beyond_small_limits, var_select = False, False, False, "first_smallest"


class InputOrder:
    has_formulas, all_neq, beyond_small_limits, var_select = False, True, True, "input_order"


def test_what_the_new_functions_do_not_do_is_refused_before_anything_runs():
    import pcp_amd.engine as E
    from pcp_amd.search_forest import forest_solutions
    for kw in (dict(objective=(0, "min")), dict(var_select="input_order"), dict(var_select="largest"), dict(sink_capacity=0), dict(sink_capacity=-3),
               dict(dist=object()), dict(brancher="widest"), dict(brancher="enumerate", val="largest"), dict(root_excl=[np.zeros((0, 2), np.int32)])):
        with pytest.raises(ValueError):
            E.Context.dfs_forest_neq_solutions(None, None, None, **kw)
    for kw in (dict(objective=(0, "min")), dict(forest="neq", var_select="input_order"), dict(var_select="largest"), dict(sink_capacity=0), dict(dist=object()),
               dict(brancher="widest"), dict(brancher="enumerate", val="largest"), dict(forest="wide")):
        with pytest.raises(ValueError):
            forest_solutions(None, None, None, **kw)
    with pytest.raises(ValueError, match="not all-XNeqY"):
        forest_solutions(NotNeq(), None, None, forest="neq")
    with pytest.raises(ValueError, match="input_order"):  # the store chooses the all-XNeqY forest and the context selects InputOrder
        forest_solutions(InputOrder(), None, None)
    with pytest.raises(ValueError, match="input_order"):
        E.Context.dfs_forest_neq_solutions(InputOrder(), None, None)


def test_the_refusals_that_were_there_before_still_stand():
    import pcp_amd.engine as E
    from pcp_amd.search_forest import forest_enumerate, forest_search
    with pytest.raises(ValueError, match="dfs_forest_neq_solutions"):
        E.Context.dfs_forest(None, None, None, collect_solutions=True)
    with pytest.raises(ValueError, match="dfs_forest_neq_solutions"):
        forest_search(None, None, None, collect_solutions=True)
    with pytest.raises(ValueError, match="dfs_forest_neq_solutions"):
        E.Context.dfs_forest_enum(None, None, None, forest="neq", collect_solutions=True)
    with pytest.raises(ValueError, match="dfs_forest_neq_solutions"):
        forest_enumerate(None, None, None, forest="neq", collect_solutions=True)
    with pytest.raises(ValueError, match="dfs_forest_enum"):
        E.Context.dfs_forest(None, None, None, brancher="enumerate")


@pytest.mark.parametrize("name", NK.CASES)
def test_the_brute_force_point_sets(name):
    sols = NK.brute(name)
    lb0, ub0 = NK.root(name)
    assert len(sols) == NK.N_SOLUTIONS[name] and all(len(p) == len(lb0) for p in sols)
    assert all(all(l <= x <= u for x, l, u in zip(p, lb0, ub0)) for p in sols)
    if name == "box":
        assert sols == NK.BOX_POINTS
    if name == "wide":
        assert len(lb0) == NK.WIDE_V == 601 and NK.WIDE_V % 64 != 0 and NK.WIDE_V > 512
        assert sorted(p[:4] for p in sols) == sorted(NK.WIDE_QUEENS)
        assert (lb0[4:] == ub0[4:]).all() and len(set(lb0[4:].tolist())) == NK.WIDE_V - 4


@pytest.mark.parametrize("name", ["queens6", "box", "wide"])
def test_the_models_are_all_xneqy_with_offsets(name):
    vs, cs = NK.build(name)
    props = cs.lower(len(vs))
    assert (props["kind"] == 0).all() and (props["var"][:, :2] < len(vs)).all()  # XNeqY over two variables: no Constant operand
    assert (props["off"] != 0).any()


def split_boxes(name):
    k = K.KeepBoxes(NK.stand_in(name))
    st = S.dfs(k, *NK.root(name), all_solutions=True)
    return st, np.stack([b[0] for b in k.boxes]), np.stack([b[1] for b in k.boxes])


def test_the_box_model_has_true_nodes_that_are_proper_boxes():
    """The oracle's search: two True nodes, each a box of four points — a row of lower bounds would name two of the eight solutions."""
    st, lbs, ubs = split_boxes("box")
    assert NK.check_boxes("box", lbs, ubs) == 2
    assert st.num_solution == 2 < NK.N_SOLUTIONS["box"] == 8
    assert sorted(int(np.prod(u - l + 1)) for l, u in zip(lbs, ubs)) == [4, 4]
    # ... and the root is no solution although a != b is entailed there: the search has to branch
    assert st.num_nodes == 3 and st.num_failed_node == 0


def test_the_wide_store_under_the_oracle():
    st, lbs, ubs = split_boxes("wide")
    assert NK.check_boxes("wide", lbs, ubs) == 0 and st.num_solution == 2
