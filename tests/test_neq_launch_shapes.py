"""Every workgroup size of the all-XNeqY kernel (pcp_neq.hip).  `neq_block` is a public option — any multiple of 64 up to 1024 — and the other
files of the suite run 256, 512 and 1024 only, the lean round 0 (neq_fast_load / neq_fast_test, neq_status_issue / neq_status_finish) at 512 and
1024 only.  That round's early status scan gives a wavefront the two nodes wv and wv + nwv and never loops: on fewer than eight wavefronts it does
not see the nodes from 2 * nwv on, and when every node it does see is open the full scan is skipped and the others are reported True.  So the lean
form is gated on eight wavefronts (neq_block >= 512), and this file pins both the results and the gate:

  * neq_block 64, 128, ..., 1024 x nodes_per_block 16, 8, 1, through the C ABI, each launch bit-exact against the oracle (Store::consistency,
    propagation/store.rs:125-164, 247-257; XNeqY x_neq_y.rs:66-104) AND against the same launch with the lean form switched off (`neq_debug` 131072);
  * pcp_debug_counters' `neq_lean` is the number of qualifying tiles at exactly the sizes `lean_may_run` names and 0 at every other: a gate that
    moves without this file being told fails here;
  * batches built so that a node either half of a wavefront is responsible for changes a status when it is skipped: (a) frontiers in which every
    node is open, (b) tiles with True / False / Unknown nodes at chosen positions, (c) tiles that narrow (quiet re-passes, whose moved nodes are
    scanned again by the same mapping), hand over to the general rounds, or fail;
  * a reduced sweep of (a) on rows of packed cells (the CELLS instantiations);
  * a listed variable without a single record that is the model's LAST variable: neq_fast_load requests the entry at its list's offset, which is
    the end of the payload table (the lowering keeps one zero entry there: tests/lower_check.cpp)."""
import numpy as np
import pytest

from oracle import oracle as orc
from pcp_amd import model as M
import pcp_amd.engine as E

from test_neq_cells import launch_cells
from util import assert_parity, dense_neq, tiles

pytestmark = pytest.mark.gpu

BLOCKS = tuple(range(64, 1025, 64))
TILE_SIZES = (16, 8, 1)
CELL_BLOCKS = (64, 256, 448, 512, 960, 1024)
LEAN_OFF = 131072       # neq_debug: the lean round 0 is not taken
K_FAST_LISTS = 4        # pcp_neq.hip kFastLists: assigned variables of a full tile up to which round 0 takes the lean form
K_FAST_PER = 6          # pcp_neq.hip kFastPer: list entries per lane of that form


def lean_may_run(nodes_per_block, neq_block, max_deg):
    """The launch shapes at which a qualifying tile takes the lean round 0 (the gate in neqfix_kernel): 16-node tiles, every list within six
    entries per lane, and at least eight wavefronts — the early status scan looks at nodes wv and wv + nwv only."""
    return nodes_per_block == 16 and max_deg <= K_FAST_PER * neq_block and neq_block >= 512


def max_degree(V, props):
    """The longest adjacency list: records per variable (LoweredInfo::max_deg), counted on the host."""
    v = props["var"][:, :2].reshape(-1)
    return int(np.bincount(v[v < V].astype(np.int64), minlength=V).max())


def lean_tiles(L, U):
    """Full 16-node tiles whose nodes have at most kFastLists assigned variables between them (what staging counts: singletons of the input rows)."""
    n_full = L.shape[0] // 16
    return sum(1 for t in range(n_full) if int((L[16 * t:16 * t + 16] == U[16 * t:16 * t + 16]).any(axis=0).sum()) <= K_FAST_LISTS)


@pytest.fixture(scope="module")
def ctx():
    c = E.Context(0)
    yield c
    c.close()


# ---- the batches: built and checked against the oracle on the host, once -----------------------------------------------------------------------
def queens_frontier(n, k_tiles=3):
    """(a) The first nodes of the reference's search on N-queens-n (the root, its children and their children in the order the search visits
    them: om.search's records), those that are Unknown, as long as the batch has at most kFastLists assigned variables; repeated up to
    16 k + 5 nodes — full tiles that qualify for the lean form and a ragged one that does not."""
    props = M.nqueens_props(n)
    om = orc.OracleModel(n, props)
    _, _, rec, _ = om.search(np.ones(n, np.int32), np.full(n, n, np.int32), all_solutions=True, node_limit=200, max_records=200)
    assigned = np.zeros(n, bool)
    keep = []
    for i in range(rec["lb_in"].shape[0]):
        a = assigned | (rec["lb_in"][i] == rec["ub_in"][i])
        if rec["status"][i] == M.UNKNOWN and (rec["lb_in"][i] <= rec["ub_in"][i]).all() and a.sum() <= K_FAST_LISTS:
            keep.append(i)
            assigned = a
        if len(keep) == 48:
            break
    N = 16 * k_tiles + 5
    idx = np.resize(np.array(keep), N)
    L, U = np.ascontiguousarray(rec["lb_in"][idx]), np.ascontiguousarray(rec["ub_in"][idx])
    ref = om.consistency(L, U, None)
    assert len(keep) >= 7 and len(set(keep)) == len(keep), keep
    assert (ref[3] == M.UNKNOWN).all(), ref[3]                        # the all-open frontier: every node Unknown ...
    assert lean_tiles(L, U) == k_tiles and assigned.sum() >= 1        # ... every full tile qualifies, and some have a list to walk
    assert n % 4 == 0                                                 # (16-byte row loads: round 0's list is built by staging)
    return dict(name=f"queens({n}) frontier", V=n, props=props, hull=(1, n), L=L, U=U, ref=ref)


B_V, B_HULL = 8, (0, 63)
B_T, B_F, B_U, B_O = "T", "F", "U", "O"  # True, False, Unknown (narrowed), open (the full domains: Unknown)
B_ARRANGEMENTS = {
    "open 0-7, T/F/U 8-15": "OOOOOOOO" "TFUTFUTF",
    "T/F/U 0-7, open 8-15": "FTUFTUFT" "OOOOOOOO",    # the first one mirrored: position p <-> 15 - p
    "Unknown at 15 only": "TFTFTFTF" "TFTFTFTU",
    # the same without failing nodes — a node that fails hands its tile to the general rounds and their full scan; these stay lean to the end
    "open 0-7, T/U 8-15": "OOOOOOOO" "TUTUTUTU",
    "T/U 0-7, open 8-15": "UTUTUTUT" "OOOOOOOO",
    "True but 15": "TTTTTTTT" "TTTTTTTU",
}


def mixed_statuses():
    """(b) 16-node tiles over a dense_neq model with True, False and Unknown nodes at chosen positions.  True: every variable in an interval of
    four values, the intervals eight apart — every record x != y + c, |c| <= 3, is entailed with no variable assigned (in every other True node
    the last variable is assigned as well); False: the two variables of the model's first record assigned to values it forbids; Unknown:
    every variable in [10, 40]; open: the full domains."""
    V, (lo, hi) = B_V, B_HULL
    props = dense_neq(31, V, B_HULL)
    om = orc.OracleModel(V, props)
    x, y, c = int(props[0]["var"][0]), int(props[0]["var"][1]), int(props[0]["off"][1])
    rows_l, rows_u, want = [], [], []
    for layout in B_ARRANGEMENTS.values():
        assert len(layout) == 16
        for p, kind in enumerate(layout):
            l, u = np.full(V, lo, np.int32), np.full(V, hi, np.int32)
            if kind == B_T:
                l, u = 8 * np.arange(V, dtype=np.int32), 8 * np.arange(V, dtype=np.int32) + 3
                if p & 2:
                    l[V - 1] = u[V - 1]
            elif kind == B_F:
                l[y] = u[y] = 20 + p
                l[x] = u[x] = 20 + p + c   # x = y + c
            elif kind == B_U:
                l[:], u[:] = 10, 40
            rows_l.append(l); rows_u.append(u)
            want.append({B_T: M.TRUE, B_F: M.FALSE}.get(kind, M.UNKNOWN))
    L, U = np.array(rows_l, np.int32), np.array(rows_u, np.int32)
    ref = om.consistency(L, U, None)
    st = ref[3].reshape(-1, 16)
    assert np.array_equal(ref[3], np.array(want, np.uint8)), (ref[3], want)   # the arrangements are what their names say
    for s in (M.TRUE, M.FALSE, M.UNKNOWN):                                    # every status on both halves of the wavefronts' node mapping
        assert (st[:, :8] == s).any() and (st[:, 8:] == s).any(), s
    assert lean_tiles(L, U) == len(B_ARRANGEMENTS)                            # every tile qualifies for the lean form
    return dict(name="mixed statuses", V=V, props=props, hull=B_HULL, L=L, U=U, ref=ref)


def narrowing_tiles(seed, V, max_assigned, p_short):
    """(c) test_neq_lean.py's tiles: nodes that narrow without assigning (quiet re-passes), that assign (hand-overs), that fail."""
    dom = (0, 20)
    props = dense_neq(100 + seed, V, dom)
    L, U = tiles(200 + seed, V, dom, 40, max_assigned, p_short)
    ref = orc.OracleModel(V, props).consistency(L, U, None)
    st = ref[3]
    changed = ((ref[0] != L) | (ref[1] != U)).any(axis=1) & (st != 0)
    newly = ((ref[0] == ref[1]) & (L != U)).any(axis=1) & (st != 0)
    assert changed.sum() > 20 and newly.sum() > 5 and (st == 0).sum() > 5 and (st == 2).sum() > 20, (int(changed.sum()), int(newly.sum()), np.bincount(st, minlength=3))
    assert lean_tiles(L, U) == 40
    return dict(name=f"narrowing tiles seed {seed}", V=V, props=props, hull=dom, L=L, U=U, ref=ref)


def isolated_last_variable():
    """A model whose last variable is in no record, assigned in some nodes of full tiles: alone (round 0's first list is its empty one) and next
    to an ordinary variable."""
    V, dom = 12, (0, 20)
    props = dense_neq(41, V - 1, dom)
    assert not (props["var"][:, :2] == V - 1).any()
    L, U = np.full((32, V), dom[0], np.int32), np.full((32, V), dom[1], np.int32)
    for b in range(0, 32, 2):
        L[b, V - 1] = U[b, V - 1] = 3 + b % 7
    for b in range(17, 32, 3):
        L[b, 3] = U[b, 3] = 5 + b % 4
    ref = orc.OracleModel(V, props).consistency(L, U, None)
    assert lean_tiles(L, U) == 2 and (ref[3] == M.UNKNOWN).all()
    return dict(name="isolated last variable", V=V, props=props, hull=dom, L=L, U=U, ref=ref)


BATCHES = {
    "a8": lambda: queens_frontier(8), "a40": lambda: queens_frontier(40), "a64": lambda: queens_frontier(64),
    "b": mixed_statuses,
    "c2": lambda: narrowing_tiles(2, 24, 2, 0.25), "c5": lambda: narrowing_tiles(5, 64, 3, 0.1),
    "last": isolated_last_variable,
}
_built = {}


def batch(key):
    if key not in _built:
        _built[key] = BATCHES[key]()
    return _built[key]


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------------
def launch_rows(ctx, L, U):
    return ctx.propagate_implicit(L, U, want_active=True)[:4]


def launch_as_cells(ctx, L, U):
    lb, ub, st = launch_cells(ctx, L.copy(), U.copy())
    return lb, ub, None, st


SEEN = {}  # neq_block -> [lean tiles, re-passes, hand-overs], summed over the sweeps on int32 rows


def sweep(ctx, bt, blocks=BLOCKS, tile_sizes=TILE_SIZES, launch=launch_rows, seen=None):
    """Every (nodes_per_block, neq_block) of the lists, lean form on and off.  The mismatches are collected and reported together."""
    V, props, L, U = bt["V"], bt["props"], bt["L"], bt["U"]
    ref = bt["ref"][:4] if launch is launch_rows else (bt["ref"][0], bt["ref"][1], None, bt["ref"][3])
    max_deg, n_lean = max_degree(V, props), lean_tiles(L, U)
    ctx.set_model(V, props)
    ctx.set_hull(*bt["hull"])
    bad = []
    try:
        for npb in tile_sizes:
            for blk in blocks:
                what = f"{bt['name']} nodes_per_block {npb} neq_block {blk}"
                got = {}
                for dbg in (0, LEAN_OFF):
                    for k, v in {"neq_path": 1, "small_path": 0, "nodes_per_block": npb, "neq_block": blk, "neq_debug": dbg}.items():
                        ctx.set_option(k, v)
                    ctx.stats_reset()
                    g = launch(ctx, L, U)
                    pl = ctx.last_plan()
                    assert (pl["path"], pl["packed"], pl["block"], pl["nodes_per_block"]) == (1, 1, blk, npb), (what, pl)
                    dc = ctx.debug_counters()
                    assert dc["neq_tiles"] == -(-L.shape[0] // npb), (what, dc)
                    want_lean = n_lean if dbg == 0 and lean_may_run(npb, blk, max_deg) else 0
                    if dc["neq_lean"] != want_lean:
                        bad.append(f"{what} neq_debug {dbg}: {dc['neq_lean']} lean tiles, expected {want_lean}")
                    if dbg == 0 and seen is not None:
                        s = seen.setdefault(blk, [0, 0, 0])
                        for i, k in enumerate(("neq_lean", "neq_lean_passes", "neq_lean_handover")):
                            s[i] += dc[k]
                    try:
                        assert_parity(ref, g, f"{what} neq_debug {dbg}")
                    except AssertionError as e:
                        bad.append(str(e))
                    got[dbg] = g
                a, b = got[0], got[LEAN_OFF]
                ok = a[3] != 0
                if not (np.array_equal(a[3], b[3]) and np.array_equal(a[0][ok], b[0][ok]) and np.array_equal(a[1][ok], b[1][ok])):
                    bad.append(f"{what}: the lean form on and off differ at nodes {np.nonzero(a[3] != b[3])[0][:10]}")
    finally:
        for k, v in {"nodes_per_block": 0, "neq_block": 0, "neq_debug": 0, "neq_path": 1, "small_path": 1}.items():
            ctx.set_option(k, v)
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad)


@pytest.mark.parametrize("key", ["a8", "a40", "a64", "b", "c2", "c5"])
def test_every_workgroup_size(ctx, key):
    sweep(ctx, batch(key), seen=SEEN)


def test_lean_branches_ran_at_and_between_the_product_sizes():
    """Over the sweeps above: lean tiles, quiet re-passes and hand-overs to the general rounds at 512 threads, at 1024 and in between."""
    for i, what in enumerate(("lean tiles", "re-passes", "hand-overs")):
        at = {blk: s[i] for blk, s in SEEN.items()}
        assert at.get(512, 0) > 0 and at.get(1024, 0) > 0 and any(at.get(blk, 0) > 0 for blk in BLOCKS if 512 < blk < 1024), (what, at)


@pytest.mark.parametrize("key", ["a8", "a40", "a64"])
def test_workgroup_sizes_on_rows_of_cells(ctx, key):
    sweep(ctx, batch(key), blocks=CELL_BLOCKS, tile_sizes=(16,), launch=launch_as_cells)


def test_listed_last_variable_without_records(ctx):
    sweep(ctx, batch("last"), blocks=(512,), tile_sizes=(16,))
