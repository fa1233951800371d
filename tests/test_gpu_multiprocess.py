"""Multi-process sharded selection with the REAL HIP kernels (VERDICT r01
item 7): two spawned ranks share cuda:0, each runs the HIP ShardedSelector on
its row shard, and the exchanges go through real torch.distributed collectives
(TorchComm over gloo -- RCCL needs one GPU per rank, see test_gpu_rccl.py for
the RCCL branch at world size 1; gloo stages the same all-gathers through the
host).  The merged selections are compared with the CPU oracle.

Covers: density-weighted select (gram mode: split-operand all-gather with the
canonical partials, each rank's own-row density with no density collective,
local exact top-k, packed top-k all-gather + merge; separable mode),
uncertainty select (no normalisation, so a zero row is accepted), and the
sharded diversity select with global candidates that all live in ONE shard
(the other rank has none).

Reference: density_weighting.py:73 (BlockMatrix shuffle), :168,:172 (sortBy +
take to the driver); similarity.py:34-38.
"""
import os
import socket

import numpy as np
import pytest

from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu

N, D, K = 5000, 64, 40


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    for p in (repo, os.path.join(repo, "distributed-active-learning_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dal import parallel
        from dal.forest import Forest

        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        X = O.synthetic_pool(N, D, seed=21)
        X[1234] = 0.0  # a zero row: legal for uncertainty sampling (rank 0's shard)
        F = Forest.synthetic(10, 4, D, seed=1)
        comm = parallel.TorchComm()
        lo, hi, _ = parallel.shard_range(N, world, rank)
        out = {}
        # uncertainty sampling over the pool with the zero row
        sel = parallel.ShardedSelector(torch.from_numpy(X[lo:hi]).to(dev), N, rank, world, device=dev)
        idx, sc = parallel.select(sel, comm, np.arange(N), F, K, mode="us")
        out["us"] = (idx.cpu().numpy(), sc.cpu().numpy())
        # density weighting (zero row replaced): gram and separable modes
        X[1234] = X[1233]
        sel = parallel.ShardedSelector(torch.from_numpy(X[lo:hi]).to(dev), N, rank, world,
                                       excluded=np.arange(10), device=dev)
        unl = np.arange(10, N)
        idx, sc = parallel.select(sel, comm, unl, F, K, mode="dw")
        out["dw"] = (idx.cpu().numpy(), sc.cpu().numpy())
        idx2, sc2 = parallel.select(sel, comm, unl, F, K, mode="dw")  # warm: cached density
        out["dw_warm"] = (idx2.cpu().numpy(), sc2.cpu().numpy())
        sel.clear_caches()
        idx, sc = parallel.select(sel, comm, unl, F, K, mode="dw", density_mode="separable")
        out["dw_sep"] = (idx.cpu().numpy(), sc.cpu().numpy())
        # sharded diversity select: candidates only in the LAST shard
        xb = torch.from_numpy(O.bf16_round(X[lo:hi])).to(dev)
        lab = torch.from_numpy(O.bf16_round(X[:128])).to(dev)
        cand = np.arange(N - 900, N)
        idx, sc = parallel.diversity_select_sharded(xb, lo, lab, 25, comm, candidates=cand, device=dev)
        out["div"] = (idx.cpu().numpy(), sc.cpu().numpy())
        q.put((rank, out))
    except Exception as e:  # surface worker failures instead of a queue timeout
        import traceback

        q.put((rank, traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_real_kernels_real_collectives(cuda):
    import torch.multiprocessing as mp

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert isinstance(r[1], dict), r[1]
    assert all(p.exitcode == 0 for p in procs)
    X = O.synthetic_pool(N, D, seed=21)
    of = O.synthetic_forest(10, 4, D, seed=1)
    X0 = X.copy()
    X0[1234] = 0.0
    _, us_idx, us_sc = O.uncertainty_select(X0, np.arange(N), of, K)
    X[1234] = X[1233]
    _, dw_idx, dw_sc = O.density_select(X, np.arange(10, N), of, K, 1.0, np.arange(10))
    Xb = O.bf16_round(X)
    cand = np.arange(N - 900, N)
    div_idx, div_sc = O.diversity_select_canonical(Xb, np.arange(128), 25, candidates=cand)
    for rank, out in res:
        assert np.array_equal(out["us"][0], us_idx) and np.array_equal(out["us"][1], us_sc), rank
        for key in ("dw", "dw_warm", "dw_sep"):
            assert np.array_equal(out[key][0], dw_idx), (rank, key)
            assert np.array_equal(out[key][1], dw_sc), (rank, key)
        assert np.array_equal(out["div"][0], div_idx), rank
        assert np.array_equal(out["div"][1], div_sc), rank


def test_bench_self_launch_two_ranks_gloo(cuda, tmp_path):
    """bench.py --gpus 2 with no outside launcher (verdict r4 item 1): the
    parent starts both ranks itself (gloo here: RCCL needs a GPU per rank),
    rank 0's headline is the parent's last stdout line, it names world_size
    2, and the timed step's self-checks (Gram selection == separable
    selection, warm == cold, bit for bit) pass on the sharded path."""
    import json
    import os
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DAL_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "2", "--config", "2", "--steps", "3",
                        "--warmup", "1", "--full", "--warm-steps", "2", "--no-cpu-baseline", "--extra", "none",
                        "--out", str(tmp_path / "full.json")],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    head = json.loads(p.stdout.strip().splitlines()[-1])
    assert head["world_size"] == 2 and head["n_gpus"] == 2 and head["backend"] == "gloo"
    assert head["self_check"]["gram_selection_equals_separable_selection"] is True
    assert head["self_check"]["warm_selection_equals_cold_selection"] is True
    assert head["ranks"]["gram_ms_max"] >= head["ranks"]["gram_ms_min"] > 0
