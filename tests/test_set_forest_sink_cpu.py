"""The set solution sink without a GPU: that the shared cases (set_forest_sink_cases.py) CAN show what a count and a row of lower bounds
lose — True nodes over IntervalSet domains that are proper products, sets with holes — and that the restatement's True nodes tile the
brute-force solution set exactly; the host side of the sink's protocol (engine.SetSolutionSink on CPU tensors); the ABI mirrors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import set_forest_sink_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("brancher,val", K.BRANCHERS)
@pytest.mark.parametrize("name", K.MODELS)
def test_true_nodes_tile_the_brute_force_set(name, brancher, val):
    """On every model, under every distributor: the products of the True nodes are pairwise disjoint and their union is the brute-force
    set.  The largest tree is 3 000 nodes or fewer (the GPU tests run each in seconds)."""
    ref = K.reference(name, brancher, val)
    assert 0 < ref["nodes"] <= 3000 and ref["solutions"] == len(ref["sets"]) > 0
    K.check_products(name, ref["sets"])


@pytest.mark.parametrize("brancher,val", K.BRANCHERS)
@pytest.mark.parametrize("name", ["rec4", "form4"])
def test_the_cases_can_show_the_loss(name, brancher, val):
    """A True node with a variable of more than one value, under each distributor: the solution count is then smaller than the number of
    solutions and the lower bounds name one point of many.  Under Enumerate rec4 also has a True node whose set has a hole (x != v took an
    interior value out)."""
    ref = K.reference(name, brancher, val)
    wide, holes = K.check_products(name, ref["sets"])
    assert wide >= 1 and ref["solutions"] < len(K.brute(name)), (wide, ref["solutions"], len(K.brute(name)))
    if name == "rec4" and brancher == "enumerate":
        assert holes >= 1


def test_the_figures_of_sched4():
    """24 True nodes, all of them points, in 61 / 89 / 67 nodes under split / Enumerate-MiddleVal / Enumerate-MinVal."""
    assert [K.counts_of("sched4", b, v)[:2] for b, v in K.BRANCHERS] == [(61, 24), (89, 24), (67, 24)]
    for b, v in K.BRANCHERS:
        assert K.check_products("sched4", K.reference("sched4", b, v)["sets"]) == (0, 0)
    assert len(K.brute("sched4")) == 24 and len(K.brute("queens6")) == 4


def test_row_shapes_cover_both_copy_paths():
    """An even and an odd number of words per row, and a row of more than one word per variable with a negative base."""
    for name in K.MODELS:
        words = K.root_bits(name).size
        assert (words % 2 == 0) == (name in K.EVEN_ROWS) and (words % 2 == 1) == (name in K.ODD_ROWS), (name, words)
    assert K.root_bits("rec2w").shape == (3, 2) and K.root_bits("rec3w").shape == (3, 3) and K.SHAPE["rec2w"][1] < 0
    assert (K.root_bits("rec2w")[2, 0] != 0) and (K.root_bits("rec2w")[2, 1] != 0)  # 60..66 from base -3 straddles the words


def test_limit_node_that_is_a_true_node():
    """A node limit at which StopNode's last node is a True node exists for rec4 (the GPU test runs it: no ticket, no row)."""
    n = K.limit_on_a_true_node("rec4")
    full, cut = K.reference("rec4"), K.reference("rec4", node_limit=n)
    assert cut["nodes"] == n and cut["statuses"][-1] == K.M.TRUE and cut["solutions"] == sum(s == K.M.TRUE for s in full["statuses"][:n]) - 1
    assert len(cut["sets"]) == cut["solutions"] >= 1


def test_set_solution_sink_bookkeeping_on_cpu_tensors():
    """drain(): min(count, capacity) rows in ticket order behind the earlier ones, the count zeroed, the overdraw kept."""
    import torch
    import pcp_amd.engine as E
    s = E.SetSolutionSink(3, 2, 2, torch.device("cpu"))
    assert s.bits.shape == (3, 2, 2) and s.struct().capacity == 3 and s.struct().reserved == 0 and s.struct().bits == s.bits.data_ptr()
    assert s.drain() == 0 and s.rows()[0].shape == (0, 2, 2) and s.rows()[0].dtype == np.uint64
    s.bits[:] = torch.arange(12).reshape(3, 2, 2)
    s.bits[0, 0, 0] = -1  # bit 63 set: comes back as an unsigned word
    s.tree[:] = torch.tensor([5, 6, 7])
    s.count[0] = 2
    assert s.drain() == 2 and int(s.count[0]) == 0 and s.overdrawn == 0
    s.count[0] = 5
    assert s.drain() == 3 and s.overdrawn == 2 and s.drains == 3
    bits, tree = s.rows()
    assert bits.shape == (5, 2, 2) and bits[0, 0, 0] == np.uint64(0xFFFFFFFFFFFFFFFF) and tree.tolist() == [5, 6, 5, 6, 7]
    assert bits[1].ravel().tolist() == [4, 5, 6, 7] and bits[4].ravel().tolist() == [8, 9, 10, 11]
    for bad in ((0, 2, 1), (1, 2, 0)):
        with pytest.raises(ValueError):
            E.SetSolutionSink(*bad, torch.device("cpu"))


def test_abi_mirrors_of_the_set_sink():
    """The header's struct, the ctypes mirror and the Rust mirror list the same fields in the same order; the symbol is declared in all
    three; the ABI number did not move (a new symbol and struct alone do not bump it)."""
    import pcp_amd.engine as E
    header = open(os.path.join(ROOT, "include", "pcp_hip.h")).read()
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*pcp_set_solution_sink\s*;", header).group(1)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == ["bits", "tree", "count", "capacity", "reserved"] == [f for f, _ in E.PcpSetSolutionSink._fields_]
    assert C.sizeof(E.PcpSetSolutionSink) == 32 and E.PcpSetSolutionSink.capacity.offset == 24
    rust = open(os.path.join(ROOT, "integration", "pcp-hip-sys", "src", "lib.rs")).read()
    rbody = re.search(r"pub struct pcp_set_solution_sink\s*\{(.*?)\n\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", re.sub(r"//[^\n]*", "", rbody)) == fields
    assert "pcp_set_solution_sink_set" in E.ABI_SYMBOLS and re.search(r"pub fn pcp_set_solution_sink_set\(", rust)
    assert re.search(r"int32_t pcp_set_solution_sink_set\(pcp_ctx\* ctx, const pcp_set_solution_sink\* sink\);", header)
    assert re.search(r"#define PCP_ABI_VERSION 8\b", header)


def test_collect_solutions_is_refused_under_branch_and_bound_and_on_several_ranks():
    """The drivers' own refusals need no device: they are raised before anything is allocated."""
    import pcp_amd.engine as E
    from pcp_amd import search_forest as SF
    with pytest.raises(ValueError, match="branch and bound"):
        E._check_collect_set("dfs_forest_set_bnb", True, 1, bnb=True)
    with pytest.raises(ValueError, match="sink_capacity"):
        E._check_collect_set("dfs_forest_set", True, 0)
    E._check_collect_set("dfs_forest_set", False, 0)
    with pytest.raises(ValueError, match="several ranks"):
        SF.forest_search_set(None, None, None, world=2, collect_solutions=True)
