"""Ranked batch-mode selection without a GPU: the numpy restatement
(tests/ranked_batch_reference.py) against its brute-force form, its properties
on the vote-weighted clustered pools (spread over the clusters, near-ties that
an fp32 decision alone would get wrong), alpha = 1 against the k-center
reference; dal.parallel.emulate_ranked_batch and ranked_batch_select_sharded
(gloo) with the local HIP steps replaced by the restatement; the weight
tables; and the argument checks of the ranked C ABI."""
import ctypes
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import kcenter_reference as KR
import ranked_batch_reference as RR
from dal import luts, parallel
from oracle import dal_oracle as O

N, D, M, K = 300, 64, 6, 20
LOW, HIGH = 37, 250  # two copies of the least similar row, in different shards, with the top weight


def _pool():
    X = KR.clustered_pool(N, D, 10, seed=N + D)
    far = O.bf16_round(-X[:M].sum(axis=0, keepdims=True))[0]  # opposite to the labeled rows
    X[LOW] = far
    X[HIGH] = far
    w = RR.lc_weights(np.random.default_rng(7).integers(0, RR.T + 1, N))
    w[LOW] = w[HIGH] = 1.0
    return X, w


_REF = {}


def _reference():
    """The one-piece selection (default alpha), computed once."""
    if not _REF:
        X, w = _pool()
        _REF["X"], _REF["w"] = X, w
        _REF["ref"] = RR.ranked_reference(X, np.arange(M), w, K, None, np.arange(M, N))
    return _REF["X"], _REF["w"], _REF["ref"]


def test_reference_equals_the_brute_force_form():
    X, w, (picks, scores, sims, m_final) = _reference()
    alpha = (N - M) / ((N - M) + M)
    c = (1.0 - alpha) * w
    live = np.zeros(N, dtype=bool)
    live[M:] = True
    got = []
    for t in range(K):
        m, _ = O.max_cosine_canonical(X, np.concatenate([np.arange(M), np.asarray(got, dtype=np.int64)]))
        g = alpha * (1.0 - m) + c
        p = int(np.argmax(np.where(live, g, -np.inf)))
        assert p == picks[t] and g[p] == scores[t] and m[p] == sims[t]
        live[p] = False
        got.append(p)
    m, _ = O.max_cosine_canonical(X, np.concatenate([np.arange(M), picks]))
    assert np.array_equal(m, m_final)
    assert picks[0] == LOW and HIGH not in picks  # after the pick its copy is the most similar row of all
    assert np.all(np.diff(scores) <= 0)


@pytest.mark.parametrize("shape", RR.SHAPES)
def test_reference_properties_on_the_weighted_pools(shape):
    from dal import _lib

    n, d, clusters, m, k = shape
    X, L, cand, w = RR.weighted_case(shape)
    picks, scores, sims, _ = RR.ranked_reference(X, L, w, k, 0.5, cand)
    assert np.all(np.diff(scores) <= 0)
    assert np.unique(picks).size == k and np.isin(picks, cand).all()
    # the plain top-k by w (ties -> lower index) stays inside the top tie group's clusters
    top = cand[np.argsort(-w[cand], kind="stable")[:k]]
    covered, plain = np.unique(picks % clusters).size, np.unique(top % clusters).size
    print(f"{shape}: clusters covered {covered} (ranked) vs {plain} (top-k by w)")
    assert covered >= 3 * plain
    # steps whose runner-up is within 2 alpha B: an fp32 decision alone picks wrongly there
    B = _lib.load().dal_kcenter_error_bound(d)
    near = int((RR.runner_up_gaps(X, L, w, k, 0.5, cand) <= 2 * 0.5 * B).sum())
    print(f"{shape}: {near} of {k} steps with the runner-up within 2 alpha B")
    if shape in (RR.SHAPES[0], RR.SHAPES[2]):
        assert near >= 10


@pytest.mark.parametrize("shape", RR.SHAPES)
def test_alpha_one_is_the_kcenter_reference(shape):
    n, d, clusters, m, k = shape
    X, L, cand, w = RR.weighted_case(shape)
    picks, scores, sims, m_final = RR.ranked_reference(X, L, w, k, 1.0, cand)
    ref = KR.kcenter_reference(X, L, k, cand)
    assert np.array_equal(picks, ref[0]) and sims.tobytes() == ref[1].tobytes()
    assert np.array_equal(m_final, ref[2]) and np.array_equal(scores, 1.0 - sims)


SIZES = {1: [N], 2: [100, 200], 3: [120, 0, 180], 5: [50, 0, 90, 100, 60]}


def _shards(X, w, P):
    bounds = np.concatenate([[0], np.cumsum(SIZES[P])])
    return ([(X[bounds[r]:bounds[r + 1]], int(bounds[r])) for r in range(P)],
            [w[bounds[r]:bounds[r + 1]] for r in range(P)])


def _assert_selection(sel, ref):
    assert np.array_equal(sel.indices.cpu().numpy(), ref[0])
    assert sel.selected_scores.cpu().numpy().tobytes() == ref[1].tobytes()
    assert sel.selected_similarity.cpu().numpy().tobytes() == ref[2].tobytes()


@pytest.mark.parametrize("P", [1, 2, 3, 5])
def test_emulate_equals_the_one_piece_reference(P):
    X, w, ref = _reference()
    shards, weights = _shards(X, w, P)
    sel = parallel.emulate_ranked_batch(shards, X[:M], weights, K, candidates=np.arange(M, N),
                                        steps=RR.NumpyRankedSteps)
    _assert_selection(sel, ref)
    assert sel.indices[0] == LOW  # the copy with the lower global index wins
    assert np.array_equal(sel.scores.numpy(), ref[3][M:])
    # an explicit alpha
    ref2 = RR.ranked_reference(X, np.arange(M), w, K, 0.3, np.arange(M, N))
    sel = parallel.emulate_ranked_batch(shards, X[:M], weights, K, alpha=0.3, candidates=np.arange(M, N),
                                        steps=RR.NumpyRankedSteps)
    _assert_selection(sel, ref2)


def test_emulate_runs_out_of_candidates_and_checks_alpha():
    X, w, _ = _reference()
    cand = np.array([5, 9, N + 3, 200, 201])  # one foreign index: the default alpha counts four
    ref = RR.ranked_reference(X, np.arange(M), w, 10, None, cand)
    assert ref[0].shape[0] == 4
    shards, weights = _shards(X, w, 3)
    sel = parallel.emulate_ranked_batch(shards, X[:M], weights, 10, candidates=cand, steps=RR.NumpyRankedSteps)
    _assert_selection(sel, ref)
    for bad in (0.0, 1.5, -1.0, float("nan"), "x"):
        with pytest.raises(ValueError, match="alpha"):
            parallel.emulate_ranked_batch(shards, X[:M], weights, 10, alpha=bad, steps=RR.NumpyRankedSteps)


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
        X, w = _pool()
        shards, weights = _shards(X, w, world)
        sel = parallel.ranked_batch_select_sharded(shards[rank][0], shards[rank][1], X[:M], weights[rank], K,
                                                   parallel.TorchComm(), candidates=np.arange(M, N),
                                                   steps=RR.NumpyRankedSteps())
        q.put((rank, sel.indices.numpy().tobytes(), sel.selected_scores.numpy().tobytes(),
               sel.selected_similarity.numpy().tobytes()))
    except Exception as e:  # surface worker failures instead of a queue timeout
        q.put((rank, repr(e), None, None))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_group_equals_the_one_piece_reference(world):
    _, _, (picks, scores, sims, _) = _reference()
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
    for rank, idx, sc, sm in res:
        assert sc is not None, idx
        assert idx == picks.tobytes() and sc == scores.tobytes() and sm == sims.tobytes(), rank


# -------------------------------------------------------------- weight LUTs --
@pytest.mark.parametrize("T", [1, 10, 100])
def test_batch_weight_luts_equal_the_stated_formulas(T):
    lc = [abs(0.5 - (1 - (v / T))) for v in range(T + 1)]
    mg = [abs((v / T) - (1 - (v / T))) for v in range(T + 1)]
    h = [0.0] + [-(v / T) * (math.log(v / T) / math.log(2)) for v in range(1, T + 1)]
    want = {"least_confidence": [1.0 - 2.0 * s for s in lc], "margin": [1.0 - s for s in mg],
            "entropy": [(0.0 + h[T - v]) + h[v] for v in range(T + 1)]}
    for strategy in luts.STRATEGIES:
        got = luts.batch_weight_lut(strategy, T)
        assert got.dtype == np.float64 and got.shape == (T + 1,)
        assert got.tobytes() == np.array(want[strategy]).tobytes()
        assert np.all((got >= 0.0) & (got <= 1.0))  # NaN-free: the one-sided entropy score is not a weight
        assert got[0] == 0.0 and got[T] == 0.0
        if T % 2 == 0:
            assert got[T // 2] == 1.0 and got.argmax() == T // 2
    with pytest.raises(ValueError):
        luts.batch_weight_lut("variance", T)


def test_batch_weights_multiclass():
    s = np.array([1.0, 0.5, 0.4, 0.0])
    assert np.array_equal(luts.batch_weights_multiclass("least_confidence", s, 3), 1.0 - s)
    assert np.array_equal(luts.batch_weights_multiclass("margin", torch.from_numpy(s), 3).numpy(), 1.0 - s)
    l3 = math.log(3) / math.log(2)
    H = np.array([0.0, 1.0, 1.5, l3, np.nextafter(l3, 2.0)])
    want = np.minimum(H / l3, 1.0)
    assert np.array_equal(luts.batch_weights_multiclass("entropy", H, 3), want)
    assert np.array_equal(luts.batch_weights_multiclass("entropy", torch.from_numpy(H), 3).numpy(), want)
    assert want[-1] == 1.0 and want[-2] == 1.0
    with pytest.raises(ValueError):
        luts.batch_weights_multiclass("variance", s, 3)


def test_default_alpha_is_formed_from_the_two_integers():
    from dal import similarity as sim

    assert sim.default_alpha(1992, 8) == 1992 / 2000 and sim.default_alpha(0, 5) == 1.0
    assert sim.check_alpha(1) == 1.0 and sim.check_alpha(2.0 ** -30) == 2.0 ** -30


# ------------------------------------------------------------------- C ABI --
def test_ranked_symbols_and_abi_version():
    from dal import _lib

    lib = _lib.load()
    assert lib.dal_abi_version() == 10
    want = {"dal_kcenter_ranked_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
            "dal_kcenter_ranked_error_bound": (ctypes.c_double, [ctypes.c_int64, ctypes.c_double]),
            "dal_kcenter_ranked_attach": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double,
                                                         ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                         ctypes.c_void_p]),
            "dal_kcenter_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])}
    for s, sig in want.items():
        assert hasattr(lib, s) and _lib.SIGNATURES[s] == sig
    for d in (64, 128, 256):
        for alpha in (1.0, 0.5, 2.0 ** -20):
            assert lib.dal_kcenter_ranked_error_bound(d, alpha) == alpha * lib.dal_kcenter_error_bound(d) + 2.0 ** -48
    assert lib.dal_kcenter_ranked_workspace_bytes(-1) == 0 and lib.dal_kcenter_ranked_workspace_bytes(1 << 31) == 0
    small, large = lib.dal_kcenter_ranked_workspace_bytes(0), lib.dal_kcenter_ranked_workspace_bytes(100000)
    assert small > 0 and small % 256 == 0 and large % 256 == 0
    assert large >= 8 * 100000 + 8 * 98 + 8 * 1024  # c[n], the block maxima, the per-wave similarities


def test_attach_and_run_reject_before_any_hip_call():
    from dal import _lib

    lib = _lib.load()
    job = ctypes.create_string_buffer(_lib.DAL_KCENTER_JOB_BYTES)
    d, m, k = 64, 4, 8
    p = {name: ctypes.c_void_p((i + 1) << 20) for i, name in enumerate(
        ("centers", "ws", "out_idx", "out_score", "status", "weight", "rws", "out_sim"))}
    need = lib.dal_kcenter_ranked_workspace_bytes(0)

    def attach(job_=job, weight=p["weight"], alpha=0.5, ws=p["rws"], wsb=need, out_sim=p["out_sim"]):
        return lib.dal_kcenter_ranked_attach(job_, weight, alpha, ws, wsb, out_sim, None)

    # an unfilled job, a null job
    assert attach() == -1 and attach(job_=None) == -1
    assert lib.dal_kcenter_run(job, None) == -1 and lib.dal_kcenter_run(None, None) == -1
    # a job over an empty shard: dal_kcenter_begin launches nothing, so the checks run without a device
    wsb = lib.dal_kcenter_workspace_bytes(0, d, m, k)
    assert lib.dal_kcenter_begin(job, None, 0, d, d, 0, None, None, None, p["centers"], m, k, p["ws"], wsb,
                                 p["out_idx"], p["out_score"], p["status"], None) == 0
    for alpha in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert attach(alpha=alpha) == -1  # DAL_ERR_ARG
    assert attach(ws=None) == -1 and attach(out_sim=None) == -1
    assert attach(wsb=need - 1) == -2 and attach(wsb=0) == -2  # DAL_ERR_SHAPE: a short workspace
    assert attach(ws=ctypes.c_void_p((7 << 20) + 128)) == -2  # not 256-B aligned
    assert attach(weight=ctypes.c_void_p((6 << 20) + 4)) == -2 and attach(out_sim=ctypes.c_void_p((8 << 20) + 4)) == -2
    # accepted: alpha = 1, and a null weight at n == 0 (nothing to launch on an empty shard)
    assert attach(alpha=1.0) == 0 and attach(weight=None) == 0
    # a refused begin leaves no job behind for attach or run
    assert lib.dal_kcenter_begin(job, None, 0, 96, 96, 0, None, None, None, p["centers"], m, k, p["ws"], wsb,
                                 p["out_idx"], p["out_score"], p["status"], None) == -2
    assert attach() == -1 and lib.dal_kcenter_run(job, None) == -1
