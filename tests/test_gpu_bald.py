"""Soft-vote BALD on the GPU: dal_forest_score_soft_bald (exact class sums,
exact sum of the leaf entropy words, the consensus entropy, score, key) and
everything above it against the restatement on Python integers and floats
(tests/bald_reference.py beside tests/soft_reference.py).

Sums, predictions and the entropy-word sums are compared bit for bit.  The
entropy is byte-identical to dal_forest_score_soft(DAL_SOFT_ENTROPY)'s, and the
score is bit for bit bald(entropy returned, hsum returned, T): one division of
two exact doubles, one subtraction, the clamp.  Against the all-Python
restatement the score is within (C + 1) 2^-49: C 2^-49 is the entropy's bound
(the device log2; tests/test_gpu_soft.py), and one more 2^-49 covers the two
roundings of the subtraction of values below 8 (2^-51 each side).  Never NaN,
never a sign bit on a zero."""
import os
import socket

import numpy as np
import pytest

import bald_cases as BC
import bald_reference as B
import soft_reference as R
import strided_pool as SP
from dal import _lib
from dal.forest import ProbabilityForest

pytestmark = pytest.mark.gpu

KEY_NONE = np.uint64(_lib.DAL_KEY_NONE)
CASES, case = BC.CASES, BC.case


def _np(t):
    return t.detach().cpu().numpy()


def _engine_bald(cuda, state, F, flags):
    import torch

    from dal import engine

    fl = None if flags is None else torch.from_numpy(np.array(flags)).to(cuda)
    s, p, hs, e, sc, k = engine.forest_score_soft_bald(state, F, fl, _lib.DAL_DESCENDING)
    _, _, e_soft, _ = engine.forest_score_soft(state, F, fl, _lib.DAL_DESCENDING, _lib.DAL_SOFT_ENTROPY)
    return _np(s), _np(p), _np(hs), _np(e), _np(sc), _np(k).view(np.uint64), _np(e_soft)


def _check_outputs(name, S, HS, flags, C, T, sums, pred, hsum, entropy, sc, keys, e_soft):
    """One launch's outputs against the restatement; e_soft: the soft entropy
    kernel's scores on the same inputs."""
    ref_S = np.array(S, dtype=np.int64)
    assert sums.dtype == np.int64 and sums.shape == ref_S.shape and np.array_equal(sums, ref_S), name
    assert pred.dtype == np.uint8 and np.array_equal(pred, R.pred(S)), name
    assert hsum.dtype == np.int64 and hsum.tolist() == HS, name
    assert entropy.dtype == np.float64 and entropy.tobytes() == e_soft.tobytes(), name
    assert sc.tobytes() == B.balds(entropy, hsum.tolist(), T).tobytes(), name
    ref = B.scores(S, HS, T)
    err = np.abs(sc - ref).max()
    print(f"{name}: max |bald_dev - bald_ref| = {err:.3e} = {err * 2.0 ** 49:.3f} x 2^-49 (bound {C + 1} x 2^-49); "
          f"{int((sc == 0).sum())} of {sc.size} scores are zero, max {sc.max():.4f}")
    assert err <= (C + 1) * 2.0 ** -49, (name, err)
    assert not np.isnan(sc).any() and (sc >= 0).all() and not np.signbit(sc).any(), name
    assert np.array_equal(keys == KEY_NONE, np.asarray(flags) == 0), name
    assert np.array_equal(keys, R.keys(sc, flags, False)), name  # the keys of the scores returned


@pytest.mark.parametrize("name", list(CASES))
def test_engine_outputs(cuda, name):
    from dal.engine import PoolState

    X, F, S, HS, flags = case(name)
    n, d, T, depth, C = CASES[name]
    state = PoolState(X, device=cuda)
    out = _engine_bald(cuda, state, F, flags)
    _check_outputs(name, S, HS, flags, C, T, *out)
    # no flags: every row is a candidate; the per-row outputs do not move
    every = _engine_bald(cuda, state, F, None)
    _check_outputs(name, S, HS, np.ones(n, dtype=np.uint8), C, T, *every)
    assert every[4].tobytes() == out[4].tobytes()
    sc = out[4]
    if name == "widest_one_hot":  # row 0 reaches one-hot leaves only
        assert out[2][0] == 0 and sc[0] == 0.0 and not np.signbit(sc[0])
    if name == "single_tree":  # H(pbar) = H(p_1): rounding only, and the clamp at work
        assert sc.max() <= 2.0 ** -29 and (sc == 0).any() and (sc > 0).any()
    else:
        assert sc.max() > 2.0 ** -20 or n == 1  # the trees do disagree


def test_paths_reached():
    """(On the CPU.)  The staging form each case is listed for
    (tests/strided_pool.py restates the tiling rule) and the side of the LDS
    budget its forest falls on (tests/bald_reference.py restates both)."""
    for name, staging in (("scalar_ragged", "scalar"), ("vec4_binary", "vec4"), ("dma_persistent", "dma"),
                          ("rows_global", "none"), ("lanes_per_row", "scalar"), ("between_budgets", "vec4")):
        n, d, T, depth, C = CASES[name]
        t = SP.forest_tiling(d, d, 4096, T)
        assert t.staging == staging, (name, t)
        assert n % t.R != 0 and n > t.R or name == "rows_global"  # more than one block, ragged last tile
    assert 256 // SP.forest_tiling(30, 30, 4096, 100).R >= 2  # several lanes per row
    assert SP.forest_tiling(300, 300, 4096, 5).R == 16 and SP.forest_tiling(256, 256, 4096, 10).R == 32
    resident = {name: B.resident(case(name)[1], True) for name in CASES}
    assert not resident["forest_global"] and not resident["between_budgets"]
    assert B.resident(case("between_budgets")[1], False)
    for name in ("scalar_ragged", "vec4_binary", "dma_persistent", "lanes_per_row", "wide_resident", "single_tree"):
        assert resident[name], name


def test_nullable_outputs_and_ascending_keys(cuda):
    """sums, pred, hsum and entropy may be null, through the C entry; ascending
    order keys the same scores the other way."""
    import torch

    for name in ("scalar_ragged", "between_budgets"):
        X, F, S, HS, flags = case(name)
        n, d, T, depth, C = CASES[name]
        x = torch.from_numpy(np.array(X)).to(cuda)
        inner, leaf_id, leaf_q = F.device(cuda)
        leaf_h = F.device_leaf_h(cuda)
        fl = torch.from_numpy(np.array(flags)).to(cuda)
        ref = B.scores(S, HS, T)
        got = {}
        for order, full in ((_lib.DAL_DESCENDING, False), (_lib.DAL_ASCENDING, True)):
            sc = torch.empty(n, dtype=torch.float64, device=cuda)
            keys = torch.empty(n, dtype=torch.int64, device=cuda)
            hsum = torch.empty(n, dtype=torch.int64, device=cuda)
            ent = torch.empty(n, dtype=torch.float64, device=cuda)
            _lib.call("dal_forest_score_soft_bald", x.data_ptr(), n, d, d, inner.data_ptr(), leaf_id.data_ptr(),
                      leaf_q.data_ptr(), leaf_h.data_ptr(), F.n_leaves, T, F.depth, C, fl.data_ptr(), order, 0, 0,
                      hsum.data_ptr() if full else 0, ent.data_ptr() if full else 0, sc.data_ptr(), keys.data_ptr(),
                      torch.cuda.current_stream(cuda).cuda_stream)
            got[full] = _np(sc)
            assert np.abs(got[full] - ref).max() <= (C + 1) * 2.0 ** -49, (name, order)
            assert np.array_equal(_np(keys).view(np.uint64), R.keys(got[full], flags, order == _lib.DAL_ASCENDING))
            if full:
                assert _np(hsum).tolist() == HS and got[full].tobytes() == B.balds(_np(ent), HS, T).tobytes()
        assert got[True].tobytes() == got[False].tobytes(), name


@pytest.mark.parametrize("name", ["scalar_ragged", "vec4_binary", "lanes_per_row", "forest_global", "single_row"])
def test_select(cuda, name):
    """uncertainty_sampling.select(strategy="bald") over the flagged rows:
    per-row outputs in unlabeled order, and for k = 1, 10 and the candidate
    count the indices are the canonical top-k of the scores the call returned."""
    from dal import uncertainty_sampling as us
    from dal.engine import PoolState

    X, F, S, HS, flags = case(name)
    n, d, T, depth, C = CASES[name]
    unl = np.nonzero(flags)[0]
    state = PoolState(X, device=cuda)
    for k in sorted({1, min(10, unl.size), unl.size}):
        sel = us.select(state, unl, F, k, strategy="bald")
        sc = _np(sel.scores)
        idx, ssc = R.topk(sc, unl, k, False)
        assert np.array_equal(_np(sel.indices), idx), (name, k)
        assert _np(sel.selected_scores).tobytes() == ssc.tobytes(), (name, k)
    assert sel.votes is None and sel.counts is None and sel.denominator == T * R.ONE
    assert np.array_equal(_np(sel.sums), np.array([S[i] for i in unl], dtype=np.int64))
    assert _np(sel.hsum).dtype == np.int64 and _np(sel.hsum).tolist() == [HS[i] for i in unl]
    assert sc.tobytes() == B.balds(_np(sel.entropy), _np(sel.hsum).tolist(), T).tobytes()
    assert np.abs(sc - B.scores([S[i] for i in unl], [HS[i] for i in unl], T)).max() <= (C + 1) * 2.0 ** -49
    # the other soft strategies carry no entropy-word sums; k above the candidate count is clamped
    assert us.select(state, unl, F, 1, strategy="entropy").hsum is None
    assert _np(us.select(state, unl, F, unl.size + 5, strategy="bald").indices).shape[0] == unl.size
    with pytest.raises(ValueError, match="ProbabilityForest"):
        us.select(state, unl, F.hard(), 1, strategy="bald")


def test_strided_unaligned_pool(cuda):
    """One pool with x_stride = d + 3 and a base 4 bytes off the allocation
    (NaN in every padding element), through the C entry: the outputs of the
    contiguous pool, and the buffer unchanged."""
    import torch

    from dal import engine
    from dal.engine import PoolState

    X, F, S, HS, flags = case("scalar_ragged")
    n, d, T, depth, C = CASES["scalar_ragged"]
    view = SP.strided(X, d + 3, 1, cuda)
    assert view.data_ptr() % 16 == 4
    inner, leaf_id, leaf_q = F.device(cuda)
    leaf_h = F.device_leaf_h(cuda)
    fl = torch.from_numpy(np.array(flags)).to(cuda)
    sums = torch.empty((n, C), dtype=torch.int64, device=cuda)
    pred = torch.empty(n, dtype=torch.uint8, device=cuda)
    hsum = torch.empty(n, dtype=torch.int64, device=cuda)
    ent = torch.empty(n, dtype=torch.float64, device=cuda)
    sc = torch.empty(n, dtype=torch.float64, device=cuda)
    keys = torch.empty(n, dtype=torch.int64, device=cuda)
    _lib.call("dal_forest_score_soft_bald", view.data_ptr(), n, d, d + 3, inner.data_ptr(), leaf_id.data_ptr(),
              leaf_q.data_ptr(), leaf_h.data_ptr(), F.n_leaves, T, F.depth, C, fl.data_ptr(), _lib.DAL_DESCENDING,
              sums.data_ptr(), pred.data_ptr(), hsum.data_ptr(), ent.data_ptr(), sc.data_ptr(), keys.data_ptr(),
              torch.cuda.current_stream(cuda).cuda_stream)
    state = PoolState(X, device=cuda)
    _, _, e_soft, _ = engine.forest_score_soft(state, F, fl, _lib.DAL_DESCENDING, _lib.DAL_SOFT_ENTROPY)
    _check_outputs("strided", S, HS, flags, C, T, _np(sums), _np(pred), _np(hsum), _np(ent), _np(sc),
                   _np(keys).view(np.uint64), _np(e_soft))
    contiguous = engine.forest_score_soft_bald(state, F, fl)
    assert _np(sc).tobytes() == _np(contiguous[4]).tobytes() and torch.equal(keys, contiguous[5])
    SP.assert_unchanged(view)


def test_select_batch_equals_ranked_batch_on_the_same_weights(cuda):
    import torch

    from dal import luts
    from dal import similarity as sim
    from dal import uncertainty_sampling as us
    from dal.engine import PoolState

    X, F, S, HS, _ = case("vec4_binary")
    n, k = X.shape[0], 12
    lab, unl = np.arange(10), np.arange(10, n)
    state = PoolState(X, device=cuda)
    sel = us.select_batch(state, unl, lab, F, k, strategy="bald", alpha=0.4)
    w_unl = _np(sel.weights)
    assert w_unl.dtype == np.float64 and w_unl.min() >= 0.0 and w_unl.max() <= 1.0 and w_unl.max() > 0.0
    one = us.select(state, unl, F, 1, strategy="bald")
    assert w_unl.tobytes() == luts.batch_weights_multiclass("bald", _np(one.scores), 2).tobytes()
    assert _np(sel.hsum).tolist() == [HS[i] for i in unl] and sel.votes is None
    w = np.zeros(n)
    w[unl] = w_unl
    simx, _ = sim._bf16_pool(torch.from_numpy(np.array(X)).to(cuda), cuda)
    ref = sim.ranked_batch_select(simx, lab, torch.from_numpy(w).to(cuda), k, alpha=0.4, candidates=unl, device=cuda)
    assert np.array_equal(_np(sel.indices), _np(ref.indices)) and np.unique(_np(sel.indices)).size == k
    assert _np(sel.selected_scores).tobytes() == _np(ref.selected_scores).tobytes()
    assert _np(sel.selected_similarity).tobytes() == _np(ref.selected_similarity).tobytes()


def test_emulated_shards_equal_the_single_device(cuda):
    """Two and three shards of one device (512-row granule: the third holds 13
    rows) merge to the single-device selection, indices and score bytes."""
    from dal import parallel
    from dal import uncertainty_sampling as us

    X, F, S, HS, flags = case("scalar_ragged")
    n, k = X.shape[0], 20
    unl = np.nonzero(flags)[0]
    one = us.select(np.array(X), unl, F, k, strategy="bald", device=cuda)
    for world in (2, 3):
        sels = []
        for r in range(world):
            lo, hi, _ = parallel.shard_range(n, world, r)
            sels.append(parallel.ShardedSelector(np.array(X[lo:hi]), n, r, world, device=cuda))
        idx, sc = parallel.emulate(sels, unl, F, k, mode="us", strategy="bald")
        assert np.array_equal(_np(idx), _np(one.indices)), world
        assert _np(sc).tobytes() == _np(one.selected_scores).tobytes(), world
    with pytest.raises(ValueError, match="ProbabilityForest"):
        parallel.emulate(sels, unl, F.hard(), k, mode="us", strategy="bald")


# ------------------------------------------------- a one-rank RCCL group --
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(port, q):
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
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        from dal import parallel
        from dal import uncertainty_sampling as us

        X, F, _, _, flags = case("scalar_ragged")
        n, k = X.shape[0], 20
        unl = np.nonzero(flags)[0]
        comm = parallel.TorchComm()
        shard = parallel.ShardedSelector(torch.from_numpy(np.array(X)).to(dev), n, 0, 1, device=dev)
        idx, sc = parallel.select(shard, comm, unl, F, k, mode="us", strategy="bald")
        one = us.select(np.array(X), unl, F, k, strategy="bald", device=dev)
        torch.cuda.synchronize()
        q.put({"backend": comm.backend, "bald": (_np(idx), _np(sc), _np(one.indices), _np(one.selected_scores))})
    except Exception:  # surface worker failures instead of a queue timeout
        import traceback

        q.put(traceback.format_exc())
        raise
    finally:
        dist.destroy_process_group()


def test_sharded_us_on_a_one_rank_nccl_group(cuda):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_free_port(), q))
    p.start()
    out = q.get(timeout=240)
    p.join(timeout=60)
    assert isinstance(out, dict), out
    assert p.exitcode == 0 and out["backend"] == "nccl"
    idx, sc, one_idx, one_sc = out["bald"]
    assert idx.shape[0] == 20 and np.array_equal(idx, one_idx)
    assert sc.tobytes() == one_sc.tobytes()


def test_run_loop_bald(cuda):
    """run_loop(strategy="bald") over a 3-class pool, scikit-learn trainer:
    three iterations, the history of the same loop with the restatement as
    select_fn."""
    from dal.loop import run_loop

    rng = np.random.default_rng(17)
    X = rng.random((400, 8)).astype(np.float32)
    y = (X[:, 0] * 3).astype(int).clip(0, 2) * 2 + 5

    def ref_select(strategy, pool, unlabeled, model, k):
        assert strategy == "bald"
        F = ProbabilityForest.from_sklearn(model)
        Xu = pool[unlabeled]
        return R.topk(B.scores(R.sums(F, Xu), B.hsums(F, Xu), F.n_trees), unlabeled, k, False)[0]

    kw = dict(strategy="bald", window_size=20, n_estimators=10, max_iterations=3, seed=4, trainer="sklearn")
    got = run_loop(X, y, device=cuda, **kw)
    ref = run_loop(X, y, select_fn=ref_select, **kw)
    assert len(got.labeled_history) == 3
    for a, b in zip(got.labeled_history, ref.labeled_history):
        assert np.array_equal(np.asarray(a), np.asarray(b))
