"""Branch and bound on the MI355X (-m gpu): pcp_propagate_device_bnb (pcp_bnb.hip around every propagation path) against the CPU oracle on
rows folded by hand, and DeviceSearch(objective=) against the restatement of the reference's loop (search/branch_and_bound.rs:64-84)."""
import ctypes as C

import numpy as np
import pytest

import pcp_amd.engine as E
from oracle import oracle as orc
from oracle_ctx import OracleCtx
from pcp_amd import model as M
from pcp_amd import search as S
from test_bnb_host import GOLOMB, _golomb, _kat_model, reference_bnb

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _solutions(V, props, lb0, ub0, k):
    """The first k solutions (lb rows, every variable assigned) of the model, from the oracle."""
    st = S.dfs(OracleCtx(V, props), lb0, ub0, all_solutions=True, node_limit=20000, batch=1)
    assert len(st.solutions) >= k
    return np.stack(st.solutions[:k])


def _fold(L, U, var, minimize, best):
    """The bound propagator folded by hand: (L, U, emptied)."""
    L, U = L.copy(), U.copy()
    if minimize:
        empty = L[:, var] > best - 1
        U[~empty, var] = np.minimum(U[~empty, var], best - 1)
    else:
        empty = U[:, var] < best + 1
        L[~empty, var] = np.maximum(L[~empty, var], best + 1)
    return L, U, empty


def _expected_reduce(lb, status, var, minimize, best):
    rows = np.nonzero(status == M.TRUE)[0]
    if not len(rows):
        return None
    v = lb[rows, var].astype(np.int64)
    r = int(rows[v.argmin() if minimize else v.argmax()])
    return r if (lb[r, var] < best if minimize else lb[r, var] > best) else None


def _run_bnb(ctx, L, U, var, mode, best, set_mode=False, base=0):
    """One pcp_propagate_device_bnb call on in-place device rows; returns host copies of everything it wrote."""
    import torch
    n, V = L.shape
    lb, ub = _t(L), _t(U)
    st = torch.zeros(n, dtype=torch.uint8, device=_dev())
    ob = {"var": var, "mode": mode, "best": _t(np.array([best], np.int32)), "best_lb": torch.full((V,), -7, dtype=torch.int32, device=_dev()),
          "best_ub": torch.full((V,), -7, dtype=torch.int32, device=_dev()), "improved": torch.zeros(1, dtype=torch.int32, device=_dev())}
    stream = torch.cuda.current_stream(_dev()).cuda_stream
    ctx.stats_reset(stream)
    if set_mode:
        bits = _t(M.interval_bits(L, U, ctx.set_words, base).view(np.int64))
        ob["best_bits"] = torch.zeros((V, ctx.set_words), dtype=torch.int64, device=_dev())
        ctx.propagate_device_bnb(n, None, None, lb, ub, None, None, st, ob, stream, bits_in=bits, bits_out=bits)
    else:
        bits = None
        ctx.propagate_device_bnb(n, lb, ub, lb, ub, None, None, st, ob, stream)
    plan = ctx.last_plan()
    ctx.stats_read(stream)  # raises PcpError on a contract violation (a hull check tripped by an emptied node)
    out = {k: (v.cpu().numpy() if v is not None else None) for k, v in ob.items() if k not in ("var", "mode")}
    out.update(lb=lb.cpu().numpy(), ub=ub.cpu().numpy(), status=st.cpu().numpy(), plan=plan,
               bits=None if bits is None else bits.cpu().numpy().view(np.uint64))
    return out


def _run_plain(ctx, L, U):
    import torch
    n = L.shape[0]
    lb, ub = _t(L), _t(U)
    st = torch.zeros(n, dtype=torch.uint8, device=_dev())
    ctx.propagate_device(n, lb, ub, lb, ub, None, None, st, torch.cuda.current_stream(_dev()).cuda_stream)
    return lb.cpu().numpy(), ub.cpu().numpy(), st.cpu().numpy()


def check_entry(ctx, om, L, U, var, want_path, bests, set_mode=False, base=0):
    """The entry's semantics on one batch, both modes: no incumbent = pcp_propagate_device (statuses, and the domains of every node that did not fail); an incumbent = the oracle on the folded
    rows, emptied nodes FALSE, the reduce (best TRUE node, lowest index on a tie, only if it beats the incumbent)."""
    for mode in ("min", "max"):
        minimize = mode == "min"
        none = E.no_incumbent(mode)
        if not set_mode:
            got = _run_bnb(ctx, L, U, var, mode, none)
            assert got["plan"]["path"] == want_path, got["plan"]
            plb, pub, pst = _run_plain(ctx, L, U)
            assert ctx.last_plan()["path"] == want_path
            ok = pst != M.FALSE  # (a failed node's domains are unspecified, include/pcp_hip.h: the assignment-driven kernel leaves them as its lanes stopped)
            assert np.array_equal(got["status"], pst) and np.array_equal(got["lb"][ok], plb[ok]) and np.array_equal(got["ub"][ok], pub[ok])
            r = _expected_reduce(plb, pst, var, minimize, none)
            assert got["best"][0] == (none if r is None else plb[r, var]) and got["improved"][0] == (r is not None)
        for best in bests[mode]:
            got = _run_bnb(ctx, L, U, var, mode, best, set_mode, base)
            assert got["plan"]["path"] == want_path, got["plan"]
            FL, FU, empty = _fold(L, U, var, minimize, best)
            if set_mode:
                fb = M.interval_bits(FL, FU, ctx.set_words, base)
                elb, eub, ebits, _, est, _ = om.consistency_set(fb[~empty], base)
            else:
                elb, eub, _, est, _ = om.consistency(FL[~empty], FU[~empty])
            st = got["status"]
            assert (st[empty] == M.FALSE).all(), mode
            assert np.array_equal(st[~empty], est), mode
            ok = est != M.FALSE
            assert np.array_equal(got["lb"][~empty][ok], elb[ok]) and np.array_equal(got["ub"][~empty][ok], eub[ok]), mode
            if set_mode:
                assert np.array_equal(got["bits"][~empty][ok], ebits[ok]), mode
            lb_all = np.zeros_like(L); lb_all[~empty] = elb
            st_all = np.zeros_like(st); st_all[~empty] = est
            r = _expected_reduce(lb_all, st_all, var, minimize, best)
            if r is None:
                assert got["best"][0] == best and got["improved"][0] == 0 and (got["best_lb"] == -7).all(), (mode, best)
            else:
                assert got["best"][0] == lb_all[r, var] and got["improved"][0] == 1, (mode, best)
                assert np.array_equal(got["best_lb"], got["lb"][r]) and np.array_equal(got["best_ub"], got["ub"][r])
                if set_mode:
                    assert np.array_equal(got["best_bits"].view(np.uint64), got["bits"][r])


def _golomb_batch(m, length, n_frontier, k_sol):
    """A Golomb batch: the BinarySplit frontier of the root, then k_sol solutions (assigned rows), the smallest ruler twice (a tie)."""
    V, props, lb0, ub0, var = _golomb(m, length)
    ctx = E.Context(0)
    ctx.set_model(V, props)
    L, U, _, _ = S.bfs_frontier(ctx, lb0, ub0, n_frontier, implicit=True)
    sols = _solutions(V, props, lb0, ub0, k_sol)
    order = np.argsort(sols[:, var], kind="stable")
    lo, hi = sols[order[0]], sols[order[-1]]
    rows_l = np.concatenate([L, sols, lo[None], hi[None]]).astype(np.int32)
    rows_u = np.concatenate([U, sols, lo[None], hi[None]]).astype(np.int32)
    return ctx, orc.OracleModel(V, props), rows_l, rows_u, var, sols


def test_entry_path4_golomb():
    ctx, om, L, U, var, sols = _golomb_batch(6, 30, 200, 24)
    vals = np.sort(sols[:, var])
    bests = {"min": [int(vals[0]), int(vals[len(vals) // 2]), int(vals[-1]) + 1, 100],
             "max": [int(vals[-1]), int(vals[len(vals) // 2]), int(vals[0]) - 1, -5]}
    check_entry(ctx, om, L, U, var, 4, bests)


def test_entry_reduce_tie_goes_to_the_lowest_index():
    import torch
    V, props, lb0, ub0, var = _golomb(6, 30)
    ctx = E.Context(0)
    ctx.set_model(V, props)
    sols = _solutions(V, props, lb0, ub0, 24)
    v = sols[:, var]
    # two different rulers of the same length: the one at the lower index wins, whichever it is
    same = [(i, j) for i in range(len(v)) for j in range(i + 1, len(v)) if v[i] == v[j] and not np.array_equal(sols[i], sols[j])]
    assert same
    i, j = same[0]
    for a, b in ((i, j), (j, i)):
        rows = np.stack([sols[a], sols[b]])
        got = _run_bnb(ctx, rows, rows, var, "min", int(v[i]) + 1)
        assert got["best"][0] == v[i] and np.array_equal(got["best_lb"], sols[a])
        got = _run_bnb(ctx, rows, rows, var, "max", int(v[i]) - 1)
        assert got["best"][0] == v[i] and np.array_equal(got["best_lb"], sols[a])
    # no TRUE node in the batch: nothing moves
    got = _run_bnb(ctx, np.stack([sols[i]]), np.stack([sols[i]]), var, "min", int(v[i]))
    assert got["status"][0] == M.FALSE and got["best"][0] == v[i] and got["improved"][0] == 0 and (got["best_lb"] == -7).all()
    del torch


def test_entry_path0_generic_kernels():
    ctx, om, L, U, var, sols = _golomb_batch(6, 30, 200, 24)
    ctx.set_option("small_path", 0)
    vals = np.sort(sols[:, var])
    check_entry(ctx, om, L, U, var, 0, {"min": [int(vals[0]), int(vals[-1]) + 1], "max": [int(vals[-1]), int(vals[0]) - 1]})


def test_entry_path1_nqueens_implicit():
    n = 8
    props = M.nqueens_props(n)
    ctx = E.Context(0)
    ctx.set_model(n, props)
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    L, U, _, _ = S.bfs_frontier(ctx, lb0, ub0, 192, implicit=True)
    sols = _solutions(n, props, lb0, ub0, 12)
    L = np.concatenate([L, sols]).astype(np.int32)
    U = np.concatenate([U, sols]).astype(np.int32)
    assert L.shape[0] >= 64
    check_entry(ctx, orc.OracleModel(n, props), L, U, 0, 1, {"min": [1, 3, 5, 9], "max": [8, 6, 4, 0]})


def test_entry_set_mode():
    n = 6
    props = M.nqueens_props(n)
    ctx = E.Context(0)
    ctx.set_model(n, props, set_words=1)
    ctx.set_hull(1, n)
    lb0, ub0 = np.ones(n, np.int32), np.full(n, n, np.int32)
    octx = E.Context(0)
    octx.set_model(n, props)
    L, U, _, _ = S.bfs_frontier(octx, lb0, ub0, 40, implicit=True)
    sols = _solutions(n, props, lb0, ub0, 4)
    L = np.concatenate([L, sols]).astype(np.int32)
    U = np.concatenate([U, sols]).astype(np.int32)
    check_entry(ctx, orc.OracleModel(n, props), L, U, 0, 0, {"min": [1, 3, 6, 7], "max": [6, 4, 1, 0]}, set_mode=True, base=1)


def test_entry_refusals():
    import torch
    V, props, lb0, ub0, var = _golomb(5, 20)
    ctx = E.Context(0)
    ctx.set_model(V, props)
    lb, ub = _t(lb0[None]), _t(ub0[None])
    st = torch.zeros(1, dtype=torch.uint8, device=_dev())
    best = _t(np.array([E.no_incumbent("min")], np.int32))
    p = lambda t: C.c_void_p(t.data_ptr())
    for cells, v, mode, want in ((1, var, 0, -5), (0, V, 0, -1), (0, var, 2, -1)):
        bt = E.DeviceBatch(p(lb), p(ub), p(lb), p(ub), None, None, p(st), None, None, None, cells, 0)
        ob = E.Objective(v, mode, p(best), None, None, None, None, 0)
        assert ctx._L.pcp_propagate_device_bnb(ctx._h, 1, C.byref(bt), C.byref(ob), None) == want, (cells, v, mode)
    torch.cuda.synchronize()


def test_device_search_batch1_is_the_reference():
    import torch
    from pcp_amd.search_device import DeviceSearch
    m, length = 7, 40
    V, props, lb0, ub0, var = _golomb(m, length)
    ref = reference_bnb(orc.OracleModel(V, props), lb0, ub0, var, True)
    g = GOLOMB[(m, length)]
    assert (ref["nodes"], ref["failed"]) == (g["nodes"], g["failed"])
    ctx = E.Context(0)
    ctx.set_model(V, props)
    ds = DeviceSearch(ctx, batch=1, capacity=4096, device=_dev(), implicit=True, objective=(var, "min"))
    st = ds.run(lb0, ub0)
    assert (st.num_nodes, st.num_failed_node, st.num_solution) == (ref["nodes"], ref["failed"], ref["solutions"])
    assert st.incumbents == ref["incumbents"] and st.incumbents[-3:] == [30, 27, 25] and st.best == 25
    assert np.array_equal(st.best_solution, ref["row"])
    del torch


def test_device_search_batched_golomb9():
    from pcp_amd.search_device import DeviceSearch
    m, length = 9, 60
    V, props, lb0, ub0, var = _golomb(m, length)
    ctx = E.Context(0)
    ctx.set_model(V, props)
    ds = DeviceSearch(ctx, batch=1024, capacity=1 << 16, device=_dev(), implicit=True, objective=(var, "min"))
    st = ds.run(lb0, ub0)
    assert st.best == GOLOMB[(m, length)]["optimum"] == 44
    assert int(ds.improved.item()) >= 1 and len(st.incumbents) == int(ds.improved.item())
    sol = st.best_solution
    _, _, _, s, _ = orc.OracleModel(V, props).consistency(sol[None], sol[None])
    assert s[0] == M.TRUE and (np.diff(sol[:m]) > 0).all() and sol[var] == 44


@pytest.mark.parametrize("mode,expect", [("max", 9), ("min", 0)])
def test_device_search_set_mode_reference_kats(mode, expect):
    from pcp_amd.search_device import DeviceSearch
    V, props, lb0, ub0, var = _kat_model()
    ctx = E.Context(0)
    ctx.set_model(V, props, set_words=1)
    ctx.set_hull(0, 10)
    for batch in (1, 4):
        st = DeviceSearch(ctx, batch=batch, capacity=256, device=_dev(), implicit=True, objective=(var, mode)).run(lb0, ub0, base=0)
        assert st.best == expect and st.best_solution[var] == expect, batch
