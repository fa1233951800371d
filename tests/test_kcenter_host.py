"""Greedy k-center selection without a GPU: the numpy restatement
(tests/kcenter_reference.py) against its brute-force form and against k
successive oracle diversity selections; dal.parallel.emulate_kcenter and
kcenter_select_sharded (gloo) with the local HIP steps replaced by the
restatement; and the argument checks of the step C ABI."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import kcenter_reference as KR
from dal import parallel
from oracle import dal_oracle as O

N, D, M, K = 300, 64, 6, 20
LOW, HIGH = 37, 250  # two copies of the least similar row, in different shards


def _pool():
    X = KR.clustered_pool(N, D, 10, seed=N + D)
    far = O.bf16_round(-X[:M].sum(axis=0, keepdims=True))[0]  # opposite to the labeled rows: the first pick
    X[LOW] = far
    X[HIGH] = far
    return X


_REF = {}


def _reference():
    """The one-piece selection, computed once."""
    if not _REF:
        X = _pool()
        _REF["X"] = X
        _REF["ref"] = KR.kcenter_reference(X, np.arange(M), K, np.arange(M, N))
    return _REF["X"], _REF["ref"]


def test_reference_equals_the_brute_force_form():
    X, (picks, values, m_final) = _reference()
    live = np.zeros(N, dtype=bool)
    live[M:] = True
    got = []
    for t in range(K):
        m, _ = O.max_cosine_canonical(X, np.concatenate([np.arange(M), np.asarray(got, dtype=np.int64)]))
        p = int(np.argmin(np.where(live, m, np.inf)))
        assert p == picks[t] and m[p] == values[t]
        live[p] = False
        got.append(p)
    m, _ = O.max_cosine_canonical(X, np.concatenate([np.arange(M), picks]))
    assert np.array_equal(m, m_final)
    assert picks[0] == LOW and HIGH not in picks  # after the pick its copy is the most similar row of all
    assert np.all(np.diff(values) >= 0)


def test_reference_equals_successive_single_picks():
    X, (picks, values, _) = _reference()
    lab, cand = list(range(M)), list(range(M, N))
    for t in range(K):
        idx, sc = O.diversity_select_canonical(X, np.asarray(lab), 1, candidates=np.asarray(cand))
        assert idx[0] == picks[t] and sc[0] == values[t]
        lab.append(int(idx[0]))
        cand.remove(int(idx[0]))


SIZES = {1: [N], 2: [100, 200], 3: [120, 0, 180], 5: [50, 0, 90, 100, 60]}


def _shards(X, P):
    bounds = np.concatenate([[0], np.cumsum(SIZES[P])])
    return [(X[bounds[r]:bounds[r + 1]], int(bounds[r])) for r in range(P)]


def _assert_selection(sel, ref):
    picks, values, _ = ref
    assert np.array_equal(sel.indices.cpu().numpy(), picks)
    assert sel.selected_scores.cpu().numpy().tobytes() == values.tobytes()


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_emulate_equals_the_one_piece_reference(P):
    X, ref = _reference()
    sel = parallel.emulate_kcenter(_shards(X, P), X[:M], K, candidates=np.arange(M, N), steps=KR.NumpyKCenterSteps)
    _assert_selection(sel, ref)
    assert sel.indices[0] == LOW  # the copy with the lower global index wins
    assert np.array_equal(sel.scores.numpy(), ref[2][M:])


def test_emulate_runs_out_of_candidates():
    X, _ = _reference()
    cand = np.array([5, 9, N + 3, 200, 201])  # one foreign index
    ref = KR.kcenter_reference(X, np.arange(M), 10, cand)
    assert ref[0].shape[0] == 4
    sel = parallel.emulate_kcenter(_shards(X, 3), X[:M], 10, candidates=cand, steps=KR.NumpyKCenterSteps)
    _assert_selection(sel, ref)


# ------------------------------------------------------------ a gloo group --
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X = _pool()
        x_local, base = _shards(X, world)[rank]
        sel = parallel.kcenter_select_sharded(x_local, base, X[:M], K, parallel.TorchComm(),
                                              candidates=np.arange(M, N), steps=KR.NumpyKCenterSteps())
        q.put((rank, sel.indices.numpy().tobytes(), sel.selected_scores.numpy().tobytes()))
    except Exception as e:  # surface worker failures instead of a queue timeout
        q.put((rank, repr(e), None))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_group_equals_the_one_piece_reference(world):
    _, (picks, values, _) = _reference()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, idx, sc in res:
        assert sc is not None, idx
        assert idx == picks.tobytes() and sc == values.tobytes(), rank


# ------------------------------------------------------------------- C ABI --
def test_kcenter_symbols_and_abi_version():
    from dal import _lib

    lib = _lib.load()
    assert lib.dal_abi_version() == 10
    for s in ("dal_kcenter_error_bound", "dal_kcenter_workspace_bytes", "dal_kcenter_begin", "dal_kcenter_propose",
              "dal_kcenter_commit", "dal_kcenter_select"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert _lib.DAL_KCENTER_JOB_BYTES == 512 and _lib.kcenter_record_bytes(128) == 32 + 256
    for d in (64, 128, 256):
        b = lib.dal_kcenter_error_bound(d)
        assert b >= lib.dal_maxcos_error_bound(d) and b > (d + 3) * 2.0 ** -24
    assert lib.dal_kcenter_workspace_bytes(1000, 96, 4, 4) == 0 and lib.dal_kcenter_workspace_bytes(1000, 64, 4, 4) > 0


def test_begin_rejects_before_any_hip_call():
    from dal import _lib

    lib = _lib.load()
    job = ctypes.create_string_buffer(_lib.DAL_KCENTER_JOB_BYTES)
    n, d, m, k = 1000, 64, 4, 8
    wsb = lib.dal_kcenter_workspace_bytes(n, d, m, k)
    rec = ctypes.c_void_p(1 << 20)

    def begin(entry="dal_kcenter_begin", null=None, **kw):
        a = dict(n=n, d=d, ld=d, m=m, k=k, wsb=wsb)
        a.update(kw)
        # placeholder addresses (aligned): every refusal below comes before a device call
        p = {name: ctypes.c_void_p((i + 1) << 20) for i, name in enumerate(
            ("pool", "flags", "m32", "inv", "centers", "ws", "out_idx", "out_score", "status"))}
        if null:
            p[null] = None
        return getattr(lib, entry)(None if null == "job" else job, p["pool"], a["n"], a["d"], a["ld"], 0, p["flags"],
                                   p["m32"], p["inv"], p["centers"], a["m"], a["k"], p["ws"], a["wsb"], p["out_idx"],
                                   p["out_score"], p["status"], None)

    for entry in ("dal_kcenter_begin", "dal_kcenter_select"):
        for d_bad in (0, 32, 96, 512):
            assert begin(entry, d=d_bad, ld=max(d_bad, 8)) == -2  # DAL_ERR_SHAPE
        assert begin(entry, m=0) == -2 and begin(entry, k=0) == -2 and begin(entry, n=-1) == -2
        assert begin(entry, ld=d - 8) == -2 and begin(entry, ld=d + 4) == -2
        assert begin(entry, wsb=wsb - 1) == -2  # a short workspace
        for name in ("job", "pool", "flags", "m32", "inv", "centers", "ws", "out_idx", "out_score", "status"):
            assert begin(entry, null=name) == -1  # DAL_ERR_ARG
        # a refused begin leaves no job behind
        assert lib.dal_kcenter_propose(job, 0, rec, None) == -1 and lib.dal_kcenter_commit(job, 0, rec, 1, None) == -1
    assert lib.dal_kcenter_propose(None, 0, rec, None) == -1
