"""Option "var_select" = PCP_VAR_INPUT_ORDER on the batched device branchers — pcp_branch_device, _hint, _excl, _set, _set_enum — against the
numpy specification (pcp_amd.search with var_select="input_order"), whose variable is checked against a scalar restatement first.  Rows
of var_select_cases: every width across the wave seam and the 256-thread stride seam, the first open variable at 0, 63, 64, 255, 256 and
V - 1 with a strictly smaller open variable behind it (FirstSmallestVar answers another index: asserted), sizes up to 2^30 - 1, batches of
1, 3 and 65 nodes with True / False / Unknown mixed.  Then the option back at 0: the FirstSmallestVar specification again.  The option
itself and the two refusals.  Integer work: no tolerance anywhere."""
import numpy as np
import pytest

import pcp_amd.engine as E
from pcp_amd import model as M
from pcp_amd import search as S

import var_select_cases as VC

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A
BATCHES = (1, 3, 65)


@pytest.fixture(scope="module")
def ctx():
    c = E.Context(0)
    yield c
    c.close()


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _up(ctx, a, view=None):
    import torch
    a = np.array(a, order="C")
    return torch.from_numpy(a.view(view) if view is not None else a).to(_dev(ctx))


def _selected(ctx, name):
    """The context under the selector `name`; the test sets it back itself."""
    ctx.var_select = name
    assert ctx.var_select == name


def _split_on_device(ctx, lb, ub, status):
    import torch
    n, V = lb.shape
    cl = torch.full((2 * n + 2, V), SENT, dtype=torch.int32, device=_dev(ctx)); cu = torch.full_like(cl, SENT)
    cd = torch.full((2 * n + 2,), SENT, dtype=torch.int32, device=_dev(ctx))
    cnt = torch.full((5,), SENT, dtype=torch.int32, device=_dev(ctx))
    t_lb, t_ub = _up(ctx, lb), _up(ctx, ub)
    ctx.branch_device(n, t_lb, t_ub, None, _up(ctx, status), cl, cu, None, cnt, child_dirty=cd)
    torch.cuda.synchronize()
    assert np.array_equal(t_lb.cpu().numpy(), lb) and np.array_equal(t_ub.cpu().numpy(), ub)  # the inputs are never written
    return cl.cpu().numpy(), cu.cpu().numpy(), cd.cpu().numpy(), cnt.cpu().numpy().tolist()


def _check_split(ctx, lb, ub, status, var_select):
    unk = status == M.UNKNOWN
    wl, wu, _ = S.branch(lb[unk], ub[unk], None, var_select=var_select)
    x = S.select_var(lb[unk], ub[unk], var_select)
    cl, cu, cd, cnt = _split_on_device(ctx, lb, ub, status)
    k = 2 * int(unk.sum())
    assert cnt == [k, int((status == M.TRUE).sum()), int((status == M.FALSE).sum()), int(unk.sum()), 0], (var_select, cnt)
    assert np.array_equal(cl[:k], wl) and np.array_equal(cu[:k], wu), var_select
    assert np.array_equal(cd[:k], np.repeat(x, 2)), (var_select, "child_dirty is the chosen variable")
    assert (cl[k:] == SENT).all() and (cu[k:] == SENT).all() and (cd[k:] == SENT).all()


def _disagreeing_rows(V):
    """var_select_cases.interval_rows, the selectors' answers checked against the scalar restatement, and the rows where they differ."""
    lb, ub, first = VC.interval_rows(V)
    size = ub.astype(np.int64) - lb.astype(np.int64) + 1
    io, fs = S.input_order(lb, ub), S.first_smallest_var(lb, ub)
    for r in range(len(lb)):
        assert io[r] == VC.ref_input_order(size[r]) == first[r] and fs[r] == VC.ref_first_smallest(size[r])
        if first[r] + 1 < V:  # a smaller open variable behind the first one: FirstSmallestVar would answer differently
            assert fs[r] == V - 1 != io[r]
    assert size.max() == 2 ** 30 - 1
    return lb, ub


@pytest.mark.parametrize("V", VC.WIDTHS)
def test_binary_split_rows_and_hints(ctx, V):
    """pcp_branch_device / _hint: the children and child_dirty under InputOrder; afterwards FirstSmallestVar's again (the option is not sticky)."""
    lb, ub = _disagreeing_rows(V)
    ctx.set_model(V, np.zeros(0, dtype=M.PROP_DTYPE))
    try:
        _selected(ctx, "input_order")
        for n in BATCHES:
            idx, status = VC.batch_of(n, len(lb))
            _check_split(ctx, lb[idx], ub[idx], status, "input_order")
    finally:
        ctx.var_select = "first_smallest"
    idx, status = VC.batch_of(3, len(lb))
    _check_split(ctx, lb[idx], ub[idx], status, "first_smallest")


def _enum_on_device(ctx, lb, ub, status, lists, val):
    import torch
    dev = _dev(ctx)
    n, V = lb.shape
    flat = np.array([tuple(p) for e in lists for p in e], np.int64).reshape(-1, 2).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(e) for e in lists])]).astype(np.int32)
    cap = 2 * len(flat) + n
    t_ex = torch.from_numpy(flat if len(flat) else np.zeros((1, 2), np.int32)).to(dev)
    cl = torch.full((2 * n, V), SENT, dtype=torch.int32, device=dev); cu = torch.full_like(cl, SENT)
    cd = torch.full((2 * n,), SENT, dtype=torch.int32, device=dev)
    coff = torch.full((2 * n + 1,), SENT, dtype=torch.int32, device=dev)
    cex = torch.full((cap + 1, 2), SENT, dtype=torch.int32, device=dev)
    cnt = torch.full((8,), SENT, dtype=torch.int32, device=dev)
    ctx.branch_device_excl(n, _up(ctx, lb), _up(ctx, ub), _up(ctx, status), torch.from_numpy(off).to(dev), t_ex, val, cl, cu, coff, cex, cap, cnt, child_dirty=cd)
    torch.cuda.synchronize()
    return cl.cpu().numpy(), cu.cpu().numpy(), cd.cpu().numpy(), coff.cpu().numpy(), cex.cpu().numpy(), cnt.cpu().numpy().tolist()


def _check_enum(ctx, lb, ub, status, val, var_select):
    """Every Unknown node carries an entry on its InputOrder variable AT the value the selector names (the existing rule must skip it), one on
    FirstSmallestVar's variable and one on a variable that is assigned."""
    unk = np.nonzero(status == M.UNKNOWN)[0]
    io = S.input_order(lb, ub)
    lists = []
    for i in range(len(lb)):
        x = int(io[i])
        v = int(lb[i, x]) if val == "min" else int(S.middle_val(lb[i:i + 1, x], ub[i:i + 1, x])[0])
        own = v + 1 if val == "min" else v  # (an excluded lower bound is no fixpoint: MinVal's own value is always free, pcp_hip.h)
        lists.append([(x, own), (lb.shape[1] - 1, 2), (x, own + 3)] if status[i] == M.UNKNOWN else [(0, 5)])
    mine = [lists[i] for i in unk]
    poff = np.concatenate([[0], np.cumsum([len(e) for e in mine])]).astype(np.int64)
    pex = np.array([p for e in mine for p in e], np.int64).reshape(-1, 2).astype(np.int32)
    x = S.select_var(lb[unk], ub[unk], var_select)
    wl, wu, woff, wex, wd = S.branch_enumerate(lb[unk], ub[unk], poff, pex, val=val, var=None if var_select == "first_smallest" else x)
    cl, cu, cd, coff, cex, cnt = _enum_on_device(ctx, lb, ub, status, lists, E.VAL_MODES[val])
    k = 2 * len(unk)
    assert cnt == [k, int((status == M.TRUE).sum()), int((status == M.FALSE).sum()), len(unk), 0, int(woff[-1]), 0, 0], (val, var_select, cnt)
    assert np.array_equal(cl[:k], wl) and np.array_equal(cu[:k], wu), (val, var_select)
    assert np.array_equal(cd[:k], wd) and np.array_equal(wd, np.repeat(x, 2)), (val, var_select)
    assert np.array_equal(coff[:k + 1], woff) and np.array_equal(cex[:int(woff[-1])], wex), (val, var_select)
    if val == "middle" and var_select == "input_order":  # the chosen variable's own excluded value was skipped: the left child sits next to it
        for j, i in enumerate(unk):
            assert cl[2 * j, io[i]] == cu[2 * j, io[i]] == lists[i][0][1] - 1


@pytest.mark.parametrize("V", VC.WIDTHS)
def test_enumerate_rows_and_lists(ctx, V):
    """pcp_branch_device_excl under InputOrder, both value selectors; then FirstSmallestVar's again."""
    lb, ub = _disagreeing_rows(V)
    ctx.set_model(V, np.zeros(0, dtype=M.PROP_DTYPE))
    try:
        _selected(ctx, "input_order")
        for n in BATCHES:
            idx, status = VC.batch_of(n, len(lb))
            for val in ("middle", "min"):
                _check_enum(ctx, lb[idx], ub[idx], status, val, "input_order")
    finally:
        ctx.var_select = "first_smallest"
    idx, status = VC.batch_of(3, len(lb))
    _check_enum(ctx, lb[idx], ub[idx], status, "middle", "first_smallest")


def _set_model(ctx, V, sw, base):
    p = np.zeros(V, dtype=M.PROP_DTYPE)
    p["kind"] = M.NEQ
    p["var"][:] = [0, M.PCP_CONST, M.PCP_NOVAR]
    p["var"][:, 0] = np.arange(V)
    p["off"][:, 1] = base
    p["group"] = np.arange(V)
    ctx.set_model(V, p, set_words=sw)
    ctx.set_hull(base, base + 64 * sw - 1)


def _sets_on_device(ctx, bits, lb, ub, status, val):
    import torch
    dev = _dev(ctx)
    n, V, sw = bits.shape
    child = torch.full((2 * n, V, sw), SENT, dtype=torch.int64, device=dev)
    cnt = torch.full((8,), SENT, dtype=torch.int32, device=dev)
    args = (n, _up(ctx, bits, np.int64), _up(ctx, lb), _up(ctx, ub), None, _up(ctx, status))
    if val is None:
        ctx.branch_device_set(*args, child, None, cnt[:5])
    else:
        ctx.branch_device_set_enum(*args, val, child, None, cnt)
    torch.cuda.synchronize()
    return child.cpu().numpy().view(np.uint64), cnt.cpu().numpy().tolist()


def _check_sets(ctx, bits, lb, ub, status, base, var_select):
    unk = status == M.UNKNOWN
    k = 2 * int(unk.sum())
    head = [k, int((status == M.TRUE).sum()), int((status == M.FALSE).sum()), int(unk.sum()), 0]
    x = S.select_var_set(bits[unk], var_select)
    want, _ = S.branch_set(bits[unk], lb[unk], ub[unk], base, None, var_select=var_select)
    got, cnt = _sets_on_device(ctx, bits, lb, ub, status, None)
    assert cnt[:5] == head and np.array_equal(got[:k], want), ("split", var_select)
    assert (got[k:] == np.uint64(SENT)).all()
    for val in ("middle", "min"):
        want, _ = S.branch_enumerate_set(bits[unk], lb[unk], ub[unk], base, None, val=val, var=None if var_select == "first_smallest" else x)
        got, cnt = _sets_on_device(ctx, bits, lb, ub, status, E.VAL_MODES[val])
        assert cnt == head + [0, 0, 0] and np.array_equal(got[:k], want), ("enumerate", val, var_select)


@pytest.mark.parametrize("V", VC.WIDTHS)
def test_set_mode_rows(ctx, V):
    """pcp_branch_device_set and _set_enum: cardinality > 1 in store order, two words per set, the first open set with holes."""
    sw, base = 2, -70
    bits, lb, ub, first = VC.set_rows(V, sw, base)
    card = S._popcount64(bits).sum(axis=2)
    io, fs = S.input_order_set(bits), S.select_var_set(bits, "first_smallest")
    for r in range(len(bits)):
        assert io[r] == VC.ref_input_order(card[r]) == first[r] and fs[r] == VC.ref_first_smallest(card[r])
        if first[r] + 1 < V:
            assert fs[r] == V - 1 != io[r]
    _set_model(ctx, V, sw, base)
    try:
        _selected(ctx, "input_order")
        for n in BATCHES:
            idx, status = VC.batch_of(n, len(bits))
            _check_sets(ctx, bits[idx], lb[idx], ub[idx], status, base, "input_order")
    finally:
        ctx.var_select = "first_smallest"
    idx, status = VC.batch_of(3, len(bits))
    _check_sets(ctx, bits[idx], lb[idx], ub[idx], status, base, "first_smallest")


def test_an_unknown_node_with_every_variable_assigned(ctx):
    """Error 3 is the same case under both selectors: pcp_branch_device writes two plain copies with the hint 0xFFFFFFFF, the Enumerate
    branchers report error 3 in counts[6]; the inputs stay untouched."""
    V = 65
    lb = np.arange(V, dtype=np.int32)[None].repeat(2, axis=0)
    status = np.array([M.UNKNOWN, M.TRUE], np.uint8)
    ctx.set_model(V, np.zeros(0, dtype=M.PROP_DTYPE))
    try:
        _selected(ctx, "input_order")
        cl, cu, cd, cnt = _split_on_device(ctx, lb, lb.copy(), status)
        assert cnt == [2, 1, 0, 1, 0] and np.array_equal(cl[:2], lb) and np.array_equal(cu[:2], lb) and (cd[:2].view(np.uint32) == 0xFFFFFFFF).all()
        *_, cnt = _enum_on_device(ctx, lb, lb.copy(), status, [[], []], E.VAL_MODES["min"])
        assert cnt[:5] == [2, 1, 0, 1, 0] and cnt[6] == 3
        sw, base = 1, 0
        _set_model(ctx, V, sw, base)
        vals = lb % 64  # (one word per set)
        _, cnt = _sets_on_device(ctx, M.interval_bits(vals, vals, sw, base), vals, vals, status, E.VAL_MODES["middle"])
        assert cnt[:5] == [2, 1, 0, 1, 0] and cnt[6] == 3
    finally:
        ctx.var_select = "first_smallest"


def test_the_option_and_the_two_refusals(ctx):
    """A value other than 0 / 1: PCP_ERR_ARG, the value before stays.  Under InputOrder pcp_dfs_forest_device and pcp_branch_device_cells
    return PCP_ERR_UNSUPPORTED with a message naming the option and launch nothing: buffers untouched, pcp_last_plan that of the launch before."""
    import torch
    dev = _dev(ctx)
    n = 6
    ctx.set_model(n, M.nqueens_props(n))
    ctx.set_hull(1, n)
    lb0, ub0 = np.ones((1, n), np.int32), np.full((1, n), n, np.int32)
    ctx.propagate(lb0, ub0)  # a launch whose plan is the one to stay
    plan = ctx.last_plan()
    try:
        _selected(ctx, "input_order")
        with pytest.raises(E.PcpError) as ei:
            ctx.set_option("var_select", 2)
        assert ei.value.code == -1 and ctx.var_select == "input_order"
        with pytest.raises(ValueError):
            ctx.var_select = "smallest"
        # the packed-cell brancher
        cells = ctx.pack_rows(_up(ctx, lb0), _up(ctx, ub0))
        torch.cuda.synchronize()
        cc = torch.full((2, n), SENT, dtype=torch.int32, device=dev)
        cd = torch.full((2,), SENT, dtype=torch.int32, device=dev)
        cnt = torch.full((5,), SENT, dtype=torch.int32, device=dev)
        with pytest.raises(E.PcpError) as ei:
            ctx.branch_device_cells(1, cells, _up(ctx, np.array([M.UNKNOWN], np.uint8)), cc, cnt, child_dirty=cd)
        assert ei.value.code == -5 and "var_select" in str(ei.value)
        torch.cuda.synchronize()
        assert (cc == SENT).all() and (cd == SENT).all() and (cnt == SENT).all()
        # the all-XNeqY in-kernel forest, through the entry itself (the drivers refuse before they get there)
        import ctypes as C
        cap = 8
        lb = torch.full((1, cap, n), SENT, dtype=torch.int32, device=dev); ub = torch.full_like(lb, SENT)
        lb[0, 0], ub[0, 0] = 1, n
        before = (lb.clone(), ub.clone())
        sp = torch.ones(1, dtype=torch.int32, device=dev); stop = torch.zeros(1, dtype=torch.int32, device=dev)
        status = torch.full((1, cap), 0x5A, dtype=torch.uint8, device=dev)
        counters = torch.zeros((1, 5), dtype=torch.int64, device=dev)
        st = E.DfsState()
        for name, t in (("lb", lb), ("ub", ub), ("sp", sp), ("stop", stop), ("status", status), ("counters", counters)):
            setattr(st, name, t.data_ptr())
        st.capacity = cap
        rc = ctx._L.pcp_dfs_forest_device(ctx._h, C.byref(st), 1, 16, 0, 0, None)
        torch.cuda.synchronize()
        assert rc == -5 and b"var_select" in ctx._L.pcp_last_error(ctx._h)
        assert torch.equal(lb, before[0]) and torch.equal(ub, before[1]) and int(sp[0]) == 1 and int(counters.sum()) == 0 and (status == 0x5A).all()
        assert ctx.last_plan() == plan
        with pytest.raises(ValueError):
            ctx.dfs_forest(lb0, ub0, var_select="input_order")
    finally:
        ctx.var_select = "first_smallest"
    assert ctx.var_select == "first_smallest"
