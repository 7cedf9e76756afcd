"""bench.py's plain run and its `--dump-outputs DIR`: the files hold what the last timed step computed (the status of every node, the
rows of a fixed sample of the nodes), in float32 / float64, small enough to keep, and the same as the engine and the oracle compute for
the same frontier."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.parametrize("explicit", [False, True])
def test_dump_step_outputs_sample_and_size(tmp_path, explicit):
    """The headline's size (16384 nodes x 1000 variables): a seeded sample of the rows, every status, at most 64 MB in all, exact values."""
    import torch
    import bench
    nodes, V, words = 16384, 1000, 16
    rng = np.random.default_rng(7)
    lb = torch.from_numpy(rng.integers(1, V + 1, (nodes, V), dtype=np.int32))
    ub = lb + torch.from_numpy(rng.integers(0, 3, (nodes, V), dtype=np.int32))
    act = torch.from_numpy(rng.integers(-2**63, 2**63 - 1, (nodes, words), dtype=np.int64)) if explicit else None
    status = torch.from_numpy(rng.integers(0, 3, nodes, dtype=np.uint8))
    bench.dump_step_outputs(str(tmp_path), (lb, ub, act), status, 0, 1)
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(["status.npy", "rows.npy", "lb.npy", "ub.npy"] + (["active.npy"] if explicit else []))
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 << 20
    out = {f[:-4]: np.load(tmp_path / f) for f in files}
    for a in out.values():
        assert a.dtype in (np.float32, np.float64)
    np.testing.assert_array_equal(out["status"], status.numpy())
    rows = out["rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_ROWS and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(out["lb"], lb.numpy()[rows])
    np.testing.assert_array_equal(out["ub"], ub.numpy()[rows])
    if explicit:
        a = act.numpy().view(np.uint64)[rows]
        got = out["active"].astype(np.uint64)
        np.testing.assert_array_equal(got[..., 0] | (got[..., 1] << np.uint64(32)), a)
    # the sample is fixed: a second dump picks the same nodes
    bench.dump_step_outputs(str(tmp_path / "again"), (lb, ub, act), status, 0, 1)
    np.testing.assert_array_equal(np.load(tmp_path / "again" / "rows.npy"), out["rows"])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    """A plain run on a small frontier: the line's headline keys, nothing of --full, and dumped outputs equal to one launch of the engine
    over the same frontier in this process (every node's status, every row of a node that did not fail) and to the oracle on a few nodes."""
    from oracle import oracle as orc
    from pcp_amd import model as M
    from pcp_amd import workloads as W
    import pcp_amd.engine as E
    import torch
    n, nodes = 1000, 2048
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--nodes", str(nodes),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "filter-steps/s" and line["higher_is_better"] is True and line["dtype"] == "i32"
    assert "cpu_baseline" not in line and "c5_nps" not in line["config"] and line["config"]["kernel_ms_per_launch"] is None
    status = np.load(tmp_path / "status.npy")
    rows = np.load(tmp_path / "rows.npy").astype(np.int64)
    glb, gub = np.load(tmp_path / "lb.npy"), np.load(tmp_path / "ub.npy")
    np.testing.assert_array_equal(rows, np.arange(nodes))  # a batch this small is written whole

    dev = torch.device("cuda", 0)
    props = M.nqueens_props(n)
    ctx = E.Context(0)
    try:
        ctx.set_model(n, props)
        ctx.set_hull(1, n)
        ctx.set_option("block_threads", 1024)  # bench.py's launch options
        ctx.set_option("nodes_per_block", 0)
        L, U, _ = W.nqueens_frontier(ctx, n, nodes, share=0, shares=8, implicit=True)
        t_lb, t_ub = torch.from_numpy(L).to(dev), torch.from_numpy(U).to(dev)
        t_st = torch.zeros(nodes, dtype=torch.uint8, device=dev)
        ctx.propagate_device(nodes, t_lb, t_ub, t_lb, t_ub, None, None, t_st)
        torch.cuda.synchronize()
        st, lb, ub = t_st.cpu().numpy(), t_lb.cpu().numpy(), t_ub.cpu().numpy()
    finally:
        ctx.close()
    np.testing.assert_array_equal(status, st.astype(np.float32))
    ok = st != 0
    np.testing.assert_array_equal(glb[ok], lb[ok].astype(np.float32))
    np.testing.assert_array_equal(gub[ok], ub[ok].astype(np.float32))
    pick = np.arange(0, nodes, nodes // 8)
    ref = orc.OracleModel(n, props).consistency(L[pick], U[pick], None, check_dup=False)
    np.testing.assert_array_equal(status[pick], ref[3].reshape(-1).astype(np.float32))
    good = ref[3].reshape(-1) != 0
    np.testing.assert_array_equal(glb[pick][good], ref[0][good].astype(np.float32))
    np.testing.assert_array_equal(gub[pick][good], ref[1][good].astype(np.float32))
