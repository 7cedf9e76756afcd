"""Enumerate in the all-XNeqY forest (pcp_dfs_forest_device_neq_enum), without a GPU: the header, the ctypes list, the built library and the
Rust bindings name the entry with pcp_dfs_forest_device_small_enum's parameter list; the drivers have the ``forest`` keyword and refuse what
that forest does not do before anything runs; and the figures test_neq_enum_forest_gpu.py compares the device with — the complete Enumerate
trees of N-queens 4, 5, 6 and 8 under the host specification (search.dfs_enumerate, batch 1, over the oracle-backed stand-in) — are pinned
and checked against TreeSim, which must re-choose values and grow the path on the MiddleVal cases the GPU tests use."""
import inspect
import os
import re

import pytest

import neq_enum_forest_cases as NC
import small_enum_forest_cases as EC
from pcp_amd import search as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (nodes, solutions, failed) of the complete Enumerate tree of N-queens-n from its root, per value selector
ENUM_TREE = {
    (4, "middle"): (11, 2, 4), (4, "min"): (11, 2, 4),
    (5, "middle"): (33, 10, 7), (5, "min"): (27, 10, 4),
    (6, "middle"): (107, 4, 50), (6, "min"): (75, 4, 34),
    (8, "middle"): (1333, 92, 575), (8, "min"): (779, 92, 298),
}


def params(header, name):
    """The parameter list of a declaration in the header, as tokens."""
    m = re.search(r"\bint32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, name
    return re.findall(r"[A-Za-z_0-9]+|\*|,", m.group(1))


def test_the_entry_is_declared_exported_and_bound_with_small_enums_parameter_list():
    """Fails without the feature: nothing names the entry, no driver has the keyword."""
    import pcp_amd.engine as E
    import pcp_amd.search_forest as SF
    import test_abi
    with open(os.path.join(ROOT, "include", "pcp_hip.h")) as f:
        header = f.read()
    name, model = "pcp_dfs_forest_device_neq_enum", "pcp_dfs_forest_device_small_enum"
    assert params(header, name) == params(header, model)
    assert re.search(r"#define\s+PCP_ABI_VERSION\s+8\b", header)
    for cite in ("enumerate.rs:33-60", "brancher.rs:52-71"):  # in the comment in front of the declaration
        doc = header[:header.index("int32_t " + name)]
        assert cite in doc[doc.rindex("/* Enumerate in the all-XNeqY forest"):]
    assert name in E.ABI_SYMBOLS and hasattr(test_abi._built(), name)
    L = E.load_library()
    assert getattr(L, name).argtypes == getattr(L, model).argtypes and getattr(L, name).restype == getattr(L, model).restype
    with open(os.path.join(ROOT, "integration", "pcp-hip-sys", "src", "lib.rs")) as f:
        rust = f.read()
    sig = lambda fn: re.sub(r"\s+", " ", re.search(r"pub fn " + fn + r"\(([^;]*)\) -> i32;", rust).group(1))
    assert sig(name) == sig(model)
    for fn in (E.Context.dfs_forest_enum, SF.forest_enumerate):
        assert inspect.signature(fn).parameters["forest"].default is None


def test_what_the_all_xneqy_forest_does_not_do_is_refused_before_anything_runs():
    import pcp_amd.engine as E
    from pcp_amd.search_forest import forest_enumerate
    for kw in (dict(forest="neq", objective=(0, "min")), dict(forest="neq", collect_solutions=True), dict(forest="neq", var_select="input_order"),
               dict(forest="neq", dist=object()), dict(forest="wide"), dict(forest="neq", val="largest")):
        with pytest.raises(ValueError):
            E.Context.dfs_forest_enum(None, None, None, **kw)
        with pytest.raises(ValueError):
            forest_enumerate(None, None, None, **kw)
    # unchanged: Enumerate through dfs_forest still needs small=True, and says where Enumerate runs otherwise
    with pytest.raises(ValueError, match="dfs_forest_enum"):
        E.Context.dfs_forest(None, None, None, brancher="enumerate")


_SPEC = {}


def spec(n, val):
    """The host specification's search, once per case."""
    if (n, val) not in _SPEC:
        _, _, lb0, ub0 = NC.queens(n)
        _SPEC[(n, val)] = S.dfs_enumerate(NC.stand_in(n), lb0, ub0, all_solutions=True, batch=1, val=val)
    return _SPEC[(n, val)]


@pytest.mark.parametrize("n,val", sorted(ENUM_TREE))
def test_the_cases_of_the_gpu_tests(n, val):
    """TreeSim gives the specification's totals on every case; under MiddleVal N-queens 5, 6 and 8 re-choose a value (the list already
    holds the selector's) and hold two or more entries on the path at once, so a device that skipped the re-choice loop or never grew
    the path could not reproduce them; MinVal never does either."""
    st = spec(n, val)
    sim = NC.TreeSim(n, val)
    assert sim.run() == EC.counts(st) == ENUM_TREE[(n, val)] and st.num_solution == NC.SOLUTIONS[n]
    assert all(NC.is_queens(s, n) for s in st.solutions)
    if val == "min":
        assert sim.rechosen == 0 and sim.max_path == 0
    elif n >= 5:
        assert sim.rechosen > 0 and sim.max_path >= 2
    else:
        assert sim.rechosen > 0 and sim.max_path == 1
