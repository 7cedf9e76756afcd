"""pcp_propagate_device_excl: nodes that carry value exclusions x != v of their own — Enumerate's right branches
(search/branching/enumerate.rs:54-59) — on the assignment-driven all-XNeqY kernel (pcp_neq.hip, the EXCL instantiations, plan.path 1).
The oracle is the judge: every node is compared with OracleModel(n, props + that node's XNeqY(x, Constant(v)) units).consistency on the same
row (the units allocated behind the model's, as Branch::distribute does, branch.rs:36-55): the status always, the rows bit-exact when the
status is not False."""
import numpy as np
import pytest

from oracle import oracle as orc
from pcp_amd import model as M
from pcp_amd import search as S
import pcp_amd.engine as E

pytestmark = pytest.mark.gpu


def _units(ex):
    """A node's exclusions as pcp_prop rows: x != Constant(v) each."""
    p = np.zeros(len(ex), dtype=M.PROP_DTYPE)
    p["kind"] = M.NEQ
    p["var"][:] = [0, M.PCP_CONST, M.PCP_NOVAR]
    p["var"][:, 0] = [int(e[0]) for e in ex]
    p["off"][:, 1] = [int(e[1]) for e in ex]
    return p


def _with_units(props, ex):
    if not len(ex):
        return props
    e = _units(ex)
    e["group"] = np.arange(len(e)) + int(props["group"].max()) + 1
    return np.concatenate([props, e])


def _oracle_nodes(n, props, L, U, excl):
    """(lb, ub, status) of every node under the oracle, each with its own exclusions; nodes without any share one model."""
    om = orc.OracleModel(n, props)
    lb, ub, st = L.copy(), U.copy(), np.zeros(len(L), np.uint8)
    for i in range(len(L)):
        m = orc.OracleModel(n, _with_units(props, excl[i])) if len(excl[i]) else om
        r = m.consistency(L[i:i + 1], U[i:i + 1], None)
        lb[i], ub[i], st[i] = r[0][0], r[1][0], r[3][0]
    return lb, ub, st


def _csr(excl):
    off = np.zeros(len(excl) + 1, np.int32)
    off[1:] = np.cumsum([len(e) for e in excl])
    flat = np.array([list(p) for e in excl for p in e], np.int64).reshape(-1, 2).astype(np.int32)
    return off, (flat if len(flat) else np.zeros((1, 2), np.int32))


def _run(ctx, L, U, excl, dirty=None):
    import torch
    dev = torch.device("cuda", 0)
    off, flat = _csr(excl)
    lb, ub = torch.from_numpy(L.copy()).to(dev), torch.from_numpy(U.copy()).to(dev)
    st = torch.full((len(L),), 255, dtype=torch.uint8, device=dev)
    d = None if dirty is None else torch.from_numpy(np.asarray(dirty, np.int32)).to(dev)
    ctx.propagate_device_excl(len(L), lb, ub, lb, ub, None, st, torch.from_numpy(off).to(dev), torch.from_numpy(flat).to(dev), dirty=d)
    assert ctx.last_plan()["path"] == 1
    torch.cuda.synchronize()
    return lb.cpu().numpy(), ub.cpu().numpy(), st.cpu().numpy()


def _check(got, ref, tag=""):
    (g_lb, g_ub, g_st), (r_lb, r_ub, r_st) = got, ref
    assert np.array_equal(g_st, r_st), (tag, np.nonzero(g_st != r_st)[0][:8], g_st[g_st != r_st][:8], r_st[g_st != r_st][:8])
    good = r_st != 0
    assert np.array_equal(g_lb[good], r_lb[good]) and np.array_equal(g_ub[good], r_ub[good]), tag


@pytest.fixture(scope="module")
def queens8():
    """The whole Enumerate / MiddleVal tree of N-queens-8, once with packed cells (declared hull) and once with int2 cells, every node recorded;
    the oracle's answer for every recorded node of the first run."""
    n = 8
    props = M.nqueens_props(n)
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    out = {"n": n, "props": props}
    for hull in (True, False):
        ctx = E.Context(0)
        try:
            ctx.set_model(n, props)
            if hull:
                ctx.set_hull(1, n)
            rec = []
            st = S.dfs_enumerate(ctx, lb0, ub0, all_solutions=True, val="middle", batch=64, record=rec)
            out[hull] = (st, rec, ctx.last_plan())
            if hull:
                out["bfs"] = S.dfs(ctx, lb0, ub0, all_solutions=True, batch=64)
        finally:
            ctx.close()
    return out


def _recorded(rec):
    L, U = np.stack([r[0] for r in rec]), np.stack([r[1] for r in rec])
    excl = [[tuple(int(x) for x in p) for p in r[2]] for r in rec]
    got = (np.stack([r[4] for r in rec]), np.stack([r[5] for r in rec]), np.array([r[3] for r in rec], np.uint8))
    return L, U, excl, got


def test_nqueens8_whole_tree_under_enumerate(queens8, golden_dir):
    import json
    import os
    import torch
    n, props = queens8["n"], queens8["props"]
    count = json.load(open(os.path.join(golden_dir, "engine_kats.json")))["search"]["all_solutions"]["counts"][n - 1]
    assert count == 92
    want = sorted(tuple(int(x) for x in s) for s in queens8["bfs"].solutions)
    assert len(want) == count
    for hull in (True, False):
        st, rec, plan = queens8[hull]
        assert plan["path"] == 1 and plan["packed"] == (1 if hull else 0)
        assert st.num_solution == count and sorted(tuple(int(x) for x in s) for s in st.solutions) == want
        L, U, excl, got = _recorded(rec)
        assert any(len(e) > 1 for e in excl)  # right branches below right branches: exclusions accumulate
        _check(got, _oracle_nodes(n, props, L, U, excl), f"hull={hull}")
    # the same nodes through the v8 entry (the one-wavefront-per-node kernel, plan.path 4): bit for bit
    L, U, excl, got = _recorded(queens8[True][1])
    off, _ = _csr(excl)
    flat = np.concatenate([_units(e) for e in excl if len(e)])
    dev = torch.device("cuda", 0)
    ctx = E.Context(0)
    try:
        ctx.set_model(n, props)
        lb, ub = torch.from_numpy(L.copy()).to(dev), torch.from_numpy(U.copy()).to(dev)
        s8 = torch.full((len(L),), 255, dtype=torch.uint8, device=dev)
        ctx.propagate_device_units(len(L), lb, ub, lb, ub, None, None, s8, torch.from_numpy(off).to(dev), torch.from_numpy(flat.view(np.uint8).copy()).to(dev))
        assert ctx.last_plan()["path"] == 4
        torch.cuda.synchronize()
        s8 = s8.cpu().numpy()
        assert np.array_equal(s8, got[2])
        good = s8 != 0
        assert np.array_equal(lb.cpu().numpy()[good], got[0][good]) and np.array_equal(ub.cpu().numpy()[good], got[1][good])
    finally:
        ctx.close()


KINDS = ("none", "interior", "chain", "conflict", "dups", "late", "badvar")
NARROWING = ("chain", "conflict", "dups", "late")


@pytest.fixture(scope="module")
def queens163():
    """N-queens-163 (not a small store; 163 >= 96 is a multiple of neither 16 nor 4 nor 2: the rows are not 16-byte aligned, the last quad and the
    last mark word are ragged): the Unknown nodes of the oracle's first 80 DFS nodes as parents, and a batch that interleaves the seven kinds of
    node — not a multiple of 16 nodes either, so the 16-node tiles end on a ragged one; the oracle's answers with and without the exclusions."""
    n = 163
    assert n >= 96 and n % 16 != 0 and n % 4 != 0
    props = M.nqueens_props(n)
    om = orc.OracleModel(n, props)
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    _, _, rec, _ = om.search(lb0, ub0, all_solutions=True, node_limit=80, max_records=80)
    unk = rec["status"] == 2
    PL, PU = rec["lb_out"][unk], rec["ub_out"][unk]
    x = S.first_smallest_var(PL, PU)
    rows = np.arange(len(x))
    v = S.middle_val(PL[rows, x], PU[rows, x])
    # the left children x = v without exclusions, at their oracle fixpoint: where a lower bound rose, an exclusion at the new bound "wakes late"
    CL, CU = PL.copy(), PU.copy()
    CL[rows, x] = v; CU[rows, x] = v
    FL, FU, _, FS, _ = om.consistency(CL, CU, None)
    L, U, excl, kind = [], [], [], []
    for i in range(len(x)):
        k = KINDS[i % len(KINDS)]
        l, u, size = PL[i], PU[i], PU[i].astype(np.int64) - PL[i] + 1
        row, ex = (l, u), None
        if k == "none":
            ex = []
        elif k == "interior" and size[x[i]] >= 3:
            ex = [(x[i], v[i] if l[x[i]] < v[i] < u[x[i]] else l[x[i]] + 1)]
        elif k == "chain":
            ys = np.nonzero(size >= 5)[0]
            if len(ys):
                y = ys[i % len(ys)]
                ex = [(y, l[y] + 1), (y, l[y] + 2), (y, l[y])]
        elif k == "conflict":
            zs = np.nonzero(size == 1)[0]
            if len(zs):
                ex = [(x[i], l[x[i]] + 1), (zs[i % len(zs)], l[zs[i % len(zs)]])] if size[x[i]] >= 3 else [(zs[0], l[zs[0]])]
        elif k == "dups":
            ex = [(x[i], l[x[i]]), (x[i], l[x[i]]), (x[i], u[x[i]]), (x[i], l[x[i]])]
        elif k == "late" and FS[i] != 0:
            ys = np.nonzero((FL[i] > CL[i]) & (FL[i] < FU[i]))[0]
            if len(ys):
                y = ys[0]
                row, ex = (CL[i], CU[i]), [(y, FL[i, y])]
        elif k == "badvar":
            ex = [(x[i], l[x[i]]), (n, 3)]
        if ex is None:
            k, ex = "none", []
        L.append(row[0]); U.append(row[1]); excl.append([(int(a), int(b)) for a, b in ex]); kind.append(k)
    if len(L) % 16 == 0:  # (the last tile of a 16-node launch must be a ragged one)
        L.pop(); U.pop(); excl.pop(); kind.pop()
    assert len(L) > 16 and len(L) % 16 != 0
    L, U = np.ascontiguousarray(np.stack(L)), np.ascontiguousarray(np.stack(U))
    kind = np.array(kind)
    ok = kind != "badvar"
    with_ex = _oracle_nodes(n, props, L, U, [e if o else [] for e, o in zip(excl, ok)])
    base = om.consistency(L, U, None)
    return {"n": n, "props": props, "L": L, "U": U, "excl": excl, "kind": kind, "ref": with_ex, "base": (base[0], base[1], base[3])}


def _check163(q, got, tag):
    ok = q["kind"] != "badvar"
    _check(tuple(a[ok] for a in got), tuple(a[ok] for a in q["ref"]), tag)
    bad = ~ok
    # a var >= n_vars refuses ITS node and no other: status none of the three, the rows untouched
    assert not np.isin(got[2][bad], (0, 1, 2)).any(), tag
    assert np.array_equal(got[0][bad], q["L"][bad]) and np.array_equal(got[1][bad], q["U"][bad]), tag


def test_nqueens163_kinds_of_node_and_launch_shapes(queens163):
    q = queens163
    kind, ref, base = q["kind"], q["ref"], q["base"]
    for k in KINDS:
        assert (kind == k).any(), k
    for k in NARROWING:  # the exclusions matter: the oracle's answer with them differs from its answer without, for a node of each kind
        sel = np.nonzero(kind == k)[0]
        assert any(ref[2][i] != base[2][i] or not np.array_equal(ref[0][i], base[0][i]) or not np.array_equal(ref[1][i], base[1][i]) for i in sel), k
    for i in np.nonzero(kind == "conflict")[0]:
        assert ref[2][i] == 0
    for i in np.nonzero(kind == "chain")[0]:
        y, l = q["excl"][i][2]
        assert ref[2][i] == 0 or ref[0][i][y] >= l + 3
    for i in np.nonzero(kind == "late")[0]:
        y, l1 = q["excl"][i][0]
        assert ref[2][i] == 0 or ref[0][i][y] > l1  # the bound ends above the excluded value it rose to
    first = None
    for hull in (True, False):
        ctx = E.Context(0)
        try:
            ctx.set_model(q["n"], q["props"])
            if hull:
                ctx.set_hull(1, q["n"])
            for npb, blk in ((0, 0), (1, 256), (16, 512), (16, 1024), (4, 64)) if hull else ((0, 0), (16, 512)):
                ctx.set_option("nodes_per_block", npb)
                ctx.set_option("neq_block", blk)
                got = _run(ctx, q["L"], q["U"], q["excl"])
                assert ctx.last_plan()["packed"] == (1 if hull else 0)
                _check163(q, got, (hull, npb, blk))
                ok = q["kind"] != "badvar"
                live = ok & (got[2] != 0)
                if first is None:
                    first = got
                assert np.array_equal(got[2][ok], first[2][ok]) and np.array_equal(got[0][live], first[0][live]) and np.array_equal(got[1][live], first[1][live])
            # the refused nodes raised the sticky flag
            with pytest.raises(E.PcpError):
                ctx.stats_read()
        finally:
            ctx.close()


def test_hinted_children_with_inherited_exclusions(queens163):
    """Left and right children of propagated parents, each with the variable it was branched on as its dirty-variable hint and exclusions
    inherited from the parent: the same result as without the hint, and the oracle's."""
    q = queens163
    n, props = q["n"], q["props"]
    om = orc.OracleModel(n, props)
    sel = np.nonzero(np.isin(q["kind"], ("none", "interior", "dups")))[0][:24]
    PL, PU, _, PS, _ = om.consistency(q["L"][sel], q["U"][sel], None)
    keep = PS == 2
    PL, PU = PL[keep], PU[keep]  # fixpoints of the model
    x = S.first_smallest_var(PL, PU)
    rows = np.arange(len(x))
    v = S.middle_val(PL[rows, x], PU[rows, x])
    CL, CU = PL.copy(), PU.copy()
    CL[rows, x] = v; CU[rows, x] = v
    FL, FU, _, FS, _ = om.consistency(CL, CU, None)
    pex = []
    for i in range(len(x)):  # inherited: interior in the parent (it is at its fixpoint with them), met by a bound once x = v propagates
        ys = [y for y in np.nonzero(FL[i] > PL[i])[0] if y != x[i] and PL[i, y] < FL[i, y] < PU[i, y]] if FS[i] != 0 else []
        e = [(int(y), int(FL[i, y])) for y in ys[:3]]
        zs = [y for y in range(n) if y != x[i] and PU[i, y] - PL[i, y] >= 2][:2]
        pex.append(e + [(int(y), int(PL[i, y]) + 1) for y in zs])
    poff, pflat = _csr(pex)
    L, U, off, ex, dirty = S.branch_enumerate(PL, PU, poff, pflat[: poff[-1]], val="middle")
    excl = [[tuple(int(t) for t in p) for p in ex[off[i]:off[i + 1]]] for i in range(len(L))]
    assert any(len(e) for e in excl[0::2]) and (dirty >= 0).all()
    ref = _oracle_nodes(n, props, L, U, excl)
    plain = om.consistency(L, U, None)
    assert not (np.array_equal(plain[0], ref[0]) and np.array_equal(plain[3], ref[2]))  # the inherited exclusions act in some child
    ctx = E.Context(0)
    try:
        ctx.set_model(n, props)
        ctx.set_hull(1, n)
        for npb in (0, 16):
            ctx.set_option("nodes_per_block", npb)
            hinted, free = _run(ctx, L, U, excl, dirty=dirty), _run(ctx, L, U, excl)
            _check(free, ref, ("no hint", npb))
            _check(hinted, ref, ("hint", npb))
    finally:
        ctx.close()


def test_several_tiles_per_workgroup(queens8):
    """2500 one-node tiles on persistent workgroups of 512 threads: every workgroup runs several tiles, each copy of a node must come out
    as its original did under the oracle."""
    n, props = queens8["n"], queens8["props"]
    L, U, excl, _ = _recorded(queens8[True][1])
    ref = _oracle_nodes(n, props, L, U, excl)
    idx = np.arange(2500) % len(L)
    ctx = E.Context(0)
    try:
        ctx.set_model(n, props)
        ctx.set_hull(1, n)
        ctx.set_option("nodes_per_block", 1)
        ctx.set_option("neq_block", 512)
        got = _run(ctx, L[idx], U[idx], [excl[i] for i in idx])
        plan = ctx.last_plan()
        assert plan["nodes_per_block"] == 1 and plan["block"] == 512 and plan["grid"] < 2500
        _check(got, tuple(a[idx] for a in ref))
    finally:
        ctx.close()


def test_refusals_and_the_plain_entry():
    import torch
    dev = torch.device("cuda", 0)
    n = 12
    props = M.nqueens_props(n)
    lb = torch.ones((4, n), dtype=torch.int32, device=dev)
    ub = torch.full((4, n), n, dtype=torch.int32, device=dev)
    st = torch.zeros(4, dtype=torch.uint8, device=dev)
    off = torch.tensor([0, 1, 1, 1, 1], dtype=torch.int32, device=dev)
    ex = torch.tensor([[0, 5]], dtype=torch.int32, device=dev)

    def refused(ctx, active_in=None, cells=False):
        # (the C entry itself: Context.propagate_device_excl offers neither explicit active rows nor packed-cell rows)
        import ctypes as C
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        bt = E.DeviceBatch(p(lb), p(ub), p(lb), p(ub), p(active_in), None, p(st), None, None, None, 1 if cells else 0, 0)
        with pytest.raises(E.PcpError) as ei:
            ctx._check(ctx._L.pcp_propagate_device_excl(ctx._h, 4, C.byref(bt), p(off), p(ex), C.c_void_p(0)))
        assert ei.value.code == -5  # PCP_ERR_UNSUPPORTED
    ctx = E.Context(0)
    try:
        ctx.set_model(n, props, set_words=1)  # set mode
        ctx.set_hull(1, n)
        refused(ctx)
        lt = np.zeros(1, dtype=M.PROP_DTYPE)  # one XLessY: not an all-XNeqY model
        lt["kind"] = M.LT
        lt["var"][0] = [0, 1, M.PCP_NOVAR]
        lt["group"] = int(props["group"].max()) + 1
        ctx.set_model(n, np.concatenate([props, lt]))
        refused(ctx)
        ctx.set_model(n, props)
        ctx.set_hull(1, n)
        refused(ctx, cells=True)
        refused(ctx, active_in=torch.full((4, ctx.words), -1, dtype=torch.int64, device=dev))
        # no offsets: exactly propagate_device
        a_lb, a_ub, a_st = lb.clone(), ub.clone(), torch.zeros(4, dtype=torch.uint8, device=dev)
        a_lb[:, 0] = 3; a_ub[:, 0] = 3
        b_lb, b_ub, b_st = a_lb.clone(), a_ub.clone(), a_st.clone()
        ctx.propagate_device_excl(4, a_lb, a_ub, a_lb, a_ub, None, a_st, None, None)
        ctx.propagate_device(4, b_lb, b_ub, b_lb, b_ub, None, None, b_st)
        torch.cuda.synchronize()
        assert torch.equal(a_lb, b_lb) and torch.equal(a_ub, b_ub) and torch.equal(a_st, b_st)
    finally:
        ctx.close()
