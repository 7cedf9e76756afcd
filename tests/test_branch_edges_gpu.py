"""pcp_branch_device_hint and pcp_branch_device_cells (branch_scan_kernel, branch_kernel, branch_cells_kernel) at their edges: every case of
branch_cases.py, in tree order and reversed, bit for bit against the scalar reference of that module — never against the other device kernel.
The child buffers, the hints and `counts` are filled with a sentinel first: what the brancher must not write still holds it afterwards.
Integer work: no tolerance anywhere."""
import numpy as np
import pytest

import pcp_amd.engine as E

import branch_cases as B

pytestmark = pytest.mark.gpu

SENT32 = 0x5A5A5A5A          # in child_lb / child_ub / child_dirty / the cells / counts
SENT64 = 0x5A5A5A5A5A5A5A5A  # in child_active
GUARD = 2                    # rows behind the 2 n the brancher may use


@pytest.fixture(scope="module")
def ctx():
    c = E.Context(0)
    yield c
    c.set_option("branch_reverse", 0)
    c.close()


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _up(ctx, a, view=None):
    import torch
    a = np.array(a, order="C")  # a copy: the cases are shared and read-only
    return torch.from_numpy(a.view(view) if view is not None else a).to(_dev(ctx))


def _ordered(e, reverse):
    """The expected children as the rows the device writes them to: child k of the batch in row n_children - 1 - k when reversed."""
    if not reverse:
        return e
    return {k: (v[::-1].copy() if isinstance(v, np.ndarray) else v) for k, v in e.items()}


def branch_rows(ctx, lb, ub, status, active, reverse, hints=True):
    """pcp_branch_device_hint over sentinel-filled buffers of 2 n + GUARD rows; returns (child_lb, child_ub, child_active, dirty, counts)."""
    import torch
    dev = _dev(ctx)
    n, V = lb.shape
    words = 0 if active is None else active.shape[1]
    rows = 2 * n + GUARD
    cl = torch.full((rows, V), SENT32, dtype=torch.int32, device=dev); cu = torch.full_like(cl, SENT32)
    ca = None if active is None else torch.full((rows, words), SENT64, dtype=torch.int64, device=dev)
    cd = torch.full((rows,), SENT32, dtype=torch.int32, device=dev) if hints else None
    cnt = torch.full((5,), SENT32, dtype=torch.int32, device=dev)
    d_act = None if active is None else _up(ctx, active, np.int64)
    ctx.set_option("branch_reverse", reverse)
    try:
        ctx.branch_device(n, _up(ctx, lb), _up(ctx, ub), d_act, _up(ctx, status), cl, cu, ca, cnt, child_dirty=cd)
        torch.cuda.synchronize()
    finally:
        ctx.set_option("branch_reverse", 0)
    return (cl.cpu().numpy(), cu.cpu().numpy(), None if ca is None else ca.cpu().numpy().view(np.uint64),
            None if cd is None else cd.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32).tolist())


def check_rows(got, e, what):
    cl, cu, ca, cd, cnt = got
    k = e["counts"][0]
    assert cnt == e["counts"], (what, cnt, e["counts"])
    assert np.array_equal(cl[:k], e["child_lb"]), (what, "child_lb", np.nonzero((cl[:k] != e["child_lb"]).any(axis=1))[0][:8])
    assert np.array_equal(cu[:k], e["child_ub"]), (what, "child_ub", np.nonzero((cu[:k] != e["child_ub"]).any(axis=1))[0][:8])
    assert (cl[k:] == SENT32).all() and (cu[k:] == SENT32).all(), (what, "rows past n_children")
    if cd is not None:
        assert np.array_equal(cd[:k], e["dirty"]), (what, "child_dirty", np.nonzero(cd[:k] != e["dirty"])[0][:8])
        assert (cd[k:] == SENT32).all(), (what, "hints past n_children")
    if ca is not None:
        assert np.array_equal(ca[:k], e["child_active"]), (what, "child_active", np.nonzero((ca[:k] != e["child_active"]).any(axis=1))[0][:8])
        assert (ca[k:] == np.uint64(SENT64)).all(), (what, "active rows past n_children")


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_rows_match_the_scalar_reference(ctx, name, reverse):
    c = B.case_by_name(name)
    V = c["lb"].shape[1]
    ctx.set_model(V, B.units_model(V, c["n_units"]))
    assert ctx.n_units == c["n_units"]
    e = _ordered(B.expected_by_name(name), reverse)
    check_rows(branch_rows(ctx, c["lb"], c["ub"], c["status"], c["active"], reverse), e, (name, reverse))
    if c["family"] == "nosplit":
        r = c["claims"]["row"]
        kids = [2 * r, 2 * r + 1] if not reverse else [e["counts"][0] - 1 - 2 * r, e["counts"][0] - 2 - 2 * r]
        cl, cu, _, cd, _ = branch_rows(ctx, c["lb"], c["ub"], c["status"], None, reverse)
        for k in kids:  # two copies of the parent, and no variable in the hint
            assert np.array_equal(cl[k], c["lb"][r]) and np.array_equal(cu[k], c["ub"][r]) and cd[k] == 0xFFFFFFFF


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("name", [n for n in B.CASE_NAMES if not n.startswith("active")])
def test_cells_match_the_scalar_reference(ctx, name, reverse):
    """The same cases as rows of packed cells, where the format can carry them: every row of the batch whose bounds lie within +-16383 (all
    of them, but for the +-(2^29 - 1) rows), without `active` rows."""
    import torch
    c = B.case_by_name(name)
    fits = B.fits_cells(c)
    if not fits.any():
        assert name == "middle-row_edge"  # nothing of this case fits the format
        return
    lb, ub, status = c["lb"][fits], c["ub"][fits], c["status"][fits]
    e = _ordered(B.expected_by_name(name) if fits.all() else B.expected(lb, ub, status), reverse)
    n, V = lb.shape
    dev = _dev(ctx)
    ctx.set_model(V, B.units_model(V, 0))
    cells = ctx.pack_rows(_up(ctx, lb), _up(ctx, ub))
    rows = 2 * n + GUARD
    cc = torch.full((rows, V), SENT32, dtype=torch.int32, device=dev)
    cd = torch.full((rows,), SENT32, dtype=torch.int32, device=dev)
    cnt = torch.full((5,), SENT32, dtype=torch.int32, device=dev)
    ctx.set_option("branch_reverse", reverse)
    try:
        ctx.branch_device_cells(n, cells, _up(ctx, status), cc, cnt, child_dirty=cd)
        torch.cuda.synchronize()
    finally:
        ctx.set_option("branch_reverse", 0)
    k = e["counts"][0]
    assert cnt.cpu().numpy().view(np.uint32).tolist() == e["counts"], (name, reverse)
    assert (cc[k:] == SENT32).all() and (cd[k:] == SENT32).all(), (name, reverse, "rows past n_children")
    assert np.array_equal(cd[:k].cpu().numpy().view(np.uint32), e["dirty"]), (name, reverse, "child_dirty")
    if k:
        l2, u2 = ctx.unpack_rows(cc[:k].contiguous())
        torch.cuda.synchronize()
        assert np.array_equal(l2.cpu().numpy(), e["child_lb"]) and np.array_equal(u2.cpu().numpy(), e["child_ub"]), (name, reverse)
    ctx.stats_read()  # nothing left the format: the sticky hull flag is down


def test_null_buffers_and_empty_batches(ctx):
    """`active` with child_active NULL, and the converse: PCP_ERR_ARG.  Both NULL on a model with units: implicit nodes, accepted.  n_nodes = 0
    zeroes counts, for rows and for cells."""
    import torch
    dev = _dev(ctx)
    c = B.case_by_name("active-65")
    V, n = c["lb"].shape[1], len(c["lb"])
    ctx.set_model(V, B.units_model(V, c["n_units"]))
    assert ctx.n_units == 65 and ctx.words == 2
    lb, ub, st, act = _up(ctx, c["lb"]), _up(ctx, c["ub"]), _up(ctx, c["status"]), _up(ctx, c["active"], np.int64)
    cl = torch.full((2 * n, V), SENT32, dtype=torch.int32, device=dev); cu = torch.full_like(cl, SENT32)
    ca = torch.full((2 * n, 2), SENT64, dtype=torch.int64, device=dev)
    cnt = torch.full((5,), SENT32, dtype=torch.int32, device=dev)
    for a, b in ((act, None), (None, ca)):
        with pytest.raises(E.PcpError) as ei:
            ctx.branch_device(n, lb, ub, a, st, cl, cu, b, cnt)
        assert ei.value.code == -1  # PCP_ERR_ARG
    torch.cuda.synchronize()
    assert (cl == SENT32).all() and (cu == SENT32).all() and (ca == SENT64).all() and (cnt == SENT32).all()  # nothing was launched
    e = B.expected(c["lb"], c["ub"], c["status"])
    check_rows(branch_rows(ctx, c["lb"], c["ub"], c["status"], None, 0), e, "implicit nodes on a model with units")
    check_rows(branch_rows(ctx, c["lb"], c["ub"], c["status"], None, 0, hints=False), e, "no hints asked for")
    ctx.branch_device(0, lb, ub, act, st, cl, cu, ca, cnt)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0] * 5 and (cl == SENT32).all() and (ca == SENT64).all()
    cnt.fill_(SENT32)
    ctx.set_model(V, B.units_model(V, 0))
    ctx.branch_device_cells(0, cl, st, cu, cnt)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0] * 5 and (cu == SENT32).all()
