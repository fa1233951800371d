"""Soft-vote forests on the GPU: dal_forest_score_soft (exact class sums,
prediction, score, key) and everything above it against the restatement on
Python integers and floats (tests/soft_reference.py).

Sums, predictions, and the least-confidence and margin scores and keys are
compared bit for bit.  The entropy carries the device log2: within C 2^-49 of
the restatement (both logs within 1 ulp; a term is at most 0.531 and takes
under 4 roundings; each of the C adds, on either side, rounds a partial sum
below 8), never -0.0 or NaN; what is selected on it is checked as the exact
canonical top-k of the scores the call returned."""
import functools
import os
import socket

import numpy as np
import pytest

import soft_reference as R
import strided_pool as SP
from dal import _lib
from dal.forest import ProbabilityForest

pytestmark = pytest.mark.gpu

KEY_NONE = np.uint64(_lib.DAL_KEY_NONE)

# name -> (n, d, T, depth, C): the smallest shape that reaches each path of the launcher
CASES = {
    "scalar_ragged": (1037, 30, 10, 4, 3),     # scalar staging, 128-row tiles, ragged last tile
    "vec4_binary": (1037, 64, 10, 4, 2),       # 16-byte staging, the binary case (class width 2)
    "dma_persistent": (517, 256, 10, 4, 10),   # LDS-DMA staging on the persistent grid, class width 16
    "rows_global": (131, 1100, 3, 2, 3),       # rows read from global memory (16 rows exceed 64 KiB)
    "lanes_per_row": (1037, 30, 100, 4, 5),    # T >= 64: several lanes per row, the cross-lane integer sum
    "widest_largest": (259, 8, 255, 3, 32),    # class width 32; one-hot leaves: some S_c = 255 2^31
    "forest_global": (523, 16, 40, 12, 4),     # synthetic, depth 12: the forest does not fit LDS
    "single_row": (1, 30, 10, 4, 3),
    "wide_resident": (300, 12, 9, 3, 21),      # class width 32 with the forest in LDS, an odd class count
    "sixteen_lanes": (67, 300, 5, 3, 6),       # 16-row tiles: 16 lanes per row, more lanes than trees or classes
}
SYNTHETIC = ("widest_largest", "forest_global")
ONE_HOT_CLASS = 7


def _np(t):
    return t.detach().cpu().numpy()


def _fitted(n, d, T, depth, C, seed):
    """A seeded pool and a scikit-learn forest fitted on its first rows (every
    class among them): ragged trees, shallow leaves, real distributions."""
    from sklearn.ensemble import RandomForestClassifier

    rng = np.random.default_rng(seed)
    X = rng.random((max(n, 200), d)).astype(np.float32)
    y = (np.floor(X[:, 0] * C).astype(int) + (X[:, 1] > 0.6)) % C
    y[:C] = np.arange(C)
    rf = RandomForestClassifier(n_estimators=T, max_depth=depth, random_state=0, n_jobs=1).fit(X[:200], y[:200])
    return X[:n], ProbabilityForest.from_sklearn(rf)


@functools.lru_cache(maxsize=None)
def case(name):
    """(X, forest, restatement sums, row flags with ~70 % candidates), computed once and never written."""
    n, d, T, depth, C = CASES[name]
    if name == "widest_largest":
        X = np.random.default_rng(5).random((n, d)).astype(np.float32)
        F = ProbabilityForest.synthetic(T, depth, d, C, seed=3)
        # the leaf row 0 reaches in every tree becomes one-hot in one class: S_c(0) = T 2^31
        hot = [(t, int(l) - t * (1 << depth), ONE_HOT_CLASS) for t, l in enumerate(R.leaf_rows(F, X[:1])[:, 0])]
        F = ProbabilityForest.synthetic(T, depth, d, C, seed=3, one_hot=hot)
    elif name == "forest_global":
        X = np.random.default_rng(6).random((n, d)).astype(np.float32)
        F = ProbabilityForest.synthetic(T, depth, d, C, seed=4)
    else:
        X, F = _fitted(n, d, T, depth, C, seed=100 + d + C)
    assert F.n_trees == T and F.n_classes == C and F.depth <= depth
    flags = (np.random.default_rng(n + d).random(n) < 0.7).astype(np.uint8)
    flags[0] = 1
    flags.setflags(write=False)
    return X, F, R.sums(F, X), flags


def _engine_score(cuda, state, F, strategy, flags):
    import torch

    from dal import engine

    fl = None if flags is None else torch.from_numpy(np.array(flags)).to(cuda)
    order = _lib.DAL_ASCENDING if R.ASCENDING[strategy] else _lib.DAL_DESCENDING
    s, p, sc, k = engine.forest_score_soft(state, F, fl, order, engine.SOFT_KINDS[strategy])
    return _np(s), _np(p), _np(sc), _np(k).view(np.uint64)


def _check_outputs(name, strategy, S, flags, C, T, sums, pred, sc, keys):
    """One launch's outputs against the restatement."""
    ref_S = np.array(S, dtype=np.int64)
    assert sums.dtype == np.int64 and sums.shape == ref_S.shape
    assert np.array_equal(sums, ref_S), (name, strategy)
    assert pred.dtype == np.uint8 and np.array_equal(pred, R.pred(S)), (name, strategy)
    ref = R.scores(S, T, strategy)
    assert np.array_equal(keys == KEY_NONE, np.asarray(flags) == 0), (name, strategy)
    assert not np.isnan(sc).any() and not np.signbit(sc[sc == 0.0]).any(), (name, strategy)
    if strategy == "entropy":
        err = np.abs(sc - ref).max()
        print(f"{name}: max |H_dev - H_ref| = {err:.3e} = {err * 2.0 ** 49:.3f} x 2^-49 (bound {C} x 2^-49)")
        assert err <= C * 2.0 ** -49, (name, err)
        assert np.array_equal(keys, R.keys(sc, flags, False)), name  # the keys of the scores returned
    else:
        assert sc.tobytes() == ref.tobytes(), (name, strategy)
        assert np.array_equal(keys, R.keys(ref, flags, True)), (name, strategy)


@pytest.mark.parametrize("name", list(CASES))
def test_engine_outputs(cuda, name):
    from dal.engine import PoolState

    X, F, S, flags = case(name)
    n, d, T, depth, C = CASES[name]
    state = PoolState(X, device=cuda)
    for strategy in R.STRATEGIES:
        _check_outputs(name, strategy, S, flags, C, T, *_engine_score(cuda, state, F, strategy, flags))
    # no flags: every row is a candidate
    _, _, sc, keys = _engine_score(cuda, state, F, "margin", None)
    assert np.array_equal(keys, R.keys(sc, np.ones(n, dtype=np.uint8), True))


def test_the_largest_sum_needs_64_bits():
    """(On the CPU first: the inputs of the widest case are what the case is for.)"""
    X, F, S, _ = case("widest_largest")
    assert S[0][ONE_HOT_CLASS] == 255 * R.ONE > 2 ** 32 and sum(S[0]) == 255 * R.ONE
    assert R.score(S[0], 255, "least_confidence") == 1.0 and R.score(S[0], 255, "entropy") == 0.0
    assert int((F.leaf_q == R.ONE).sum()) >= 1


def test_paths_reached():
    """The staging form each case is listed for (tests/strided_pool.py restates the tiling rule)."""
    for name, staging in (("scalar_ragged", "scalar"), ("vec4_binary", "vec4"), ("dma_persistent", "dma"),
                          ("rows_global", "none"), ("lanes_per_row", "scalar")):
        n, d, T, depth, C = CASES[name]
        t = SP.forest_tiling(d, d, 4096, T)
        assert t.staging == staging, (name, t)
        assert n % t.R != 0 and n > t.R or name == "rows_global"  # more than one block, ragged last tile
    assert 256 // SP.forest_tiling(30, 30, 4096, 100).R >= 2  # several lanes per row
    assert SP.forest_tiling(300, 300, 4096, 5).R == 16 and SP.forest_tiling(256, 256, 4096, 10).R == 32
    X, F, _, _ = case("forest_global")
    assert F.n_trees * (((1 << F.depth) - 1) * 8 + (1 << F.depth) * 4) > 65536


@pytest.mark.parametrize("name", list(CASES))
def test_select(cuda, name):
    """uncertainty_sampling.select over the flagged rows: per-row outputs in
    unlabeled order, and for k = 1, 10 and the candidate count the indices are
    the canonical top-k of the scores the call returned (for least confidence
    and margin also the restatement's selection, bit for bit)."""
    from dal import uncertainty_sampling as us
    from dal.engine import PoolState

    X, F, S, flags = case(name)
    n, d, T, depth, C = CASES[name]
    unl = np.nonzero(flags)[0]
    S_unl = [S[i] for i in unl]
    state = PoolState(X, device=cuda)
    for strategy in R.STRATEGIES:
        for k in sorted({1, min(10, unl.size), unl.size}):
            sel = us.select(state, unl, F, k, strategy=strategy)
            sc = _np(sel.scores)
            idx, ssc = R.topk(sc, unl, k, R.ASCENDING[strategy])
            assert np.array_equal(_np(sel.indices), idx), (name, strategy, k)
            assert _np(sel.selected_scores).tobytes() == ssc.tobytes(), (name, strategy, k)
            if strategy != "entropy":
                ref_idx, ref_sc = R.select(S_unl, T, strategy, unl, k)
                assert np.array_equal(_np(sel.indices), ref_idx) and _np(sel.selected_scores).tobytes() == ref_sc.tobytes()
        assert sel.votes is None and sel.counts is None and sel.denominator == T * R.ONE
        assert np.array_equal(_np(sel.sums), np.array(S_unl, dtype=np.int64)), (name, strategy)
        assert _np(sel.proba()).tobytes() == R.proba(S_unl, T).tobytes(), (name, strategy)
        if strategy != "entropy":
            assert sc.tobytes() == R.scores(S_unl, T, strategy).tobytes()
    # k above the candidate count is clamped
    assert _np(us.select(state, unl, F, unl.size + 5).indices).shape[0] == unl.size


def test_strided_unaligned_pool(cuda):
    """One pool with x_stride = d + 3 and a base 4 bytes off the allocation
    (NaN in every padding element), through the C entry: the outputs of the
    contiguous pool, and the buffer unchanged."""
    import torch

    X, F, S, flags = case("scalar_ragged")
    n, d, T, depth, C = CASES["scalar_ragged"]
    view = SP.strided(X, d + 3, 1, cuda)
    assert view.data_ptr() % 16 == 4
    inner, leaf_id, leaf_q = F.device(cuda)
    fl = torch.from_numpy(np.array(flags)).to(cuda)
    for strategy in R.STRATEGIES:
        sums = torch.empty((n, C), dtype=torch.int64, device=cuda)
        pred = torch.empty(n, dtype=torch.uint8, device=cuda)
        sc = torch.empty(n, dtype=torch.float64, device=cuda)
        keys = torch.empty(n, dtype=torch.int64, device=cuda)
        kind = {"least_confidence": 0, "margin": 1, "entropy": 2}[strategy]
        order = _lib.DAL_ASCENDING if R.ASCENDING[strategy] else _lib.DAL_DESCENDING
        _lib.call("dal_forest_score_soft", view.data_ptr(), n, d, d + 3, inner.data_ptr(), leaf_id.data_ptr(),
                  leaf_q.data_ptr(), F.n_leaves, T, F.depth, C, kind, fl.data_ptr(), order, sums.data_ptr(),
                  pred.data_ptr(), sc.data_ptr(), keys.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream)
        _check_outputs("strided", strategy, S, flags, C, T, _np(sums), _np(pred), _np(sc), _np(keys).view(np.uint64))
    SP.assert_unchanged(view)


def test_predict_proba(cuda):
    from dal import random_forest

    for name in ("scalar_ragged", "widest_largest"):
        X, F, S, _ = case(name)
        T = CASES[name][2]
        proba, pred = random_forest.predict_proba(F, X, device=cuda)
        assert _np(proba).dtype == np.float64 and _np(proba).tobytes() == R.proba(S, T).tobytes()
        assert np.array_equal(_np(pred), R.pred(S))
        p2, sums = random_forest.predict(F, X, device=cuda)
        assert np.array_equal(_np(p2), R.pred(S)) and np.array_equal(_np(sums), np.array(S, dtype=np.int64))
    assert _np(proba)[0, ONE_HOT_CLASS] == 1.0
    with pytest.raises(ValueError, match="ProbabilityForest"):
        random_forest.predict_proba(F.hard(), X, device=cuda)


@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_select_batch_equals_ranked_batch_on_the_same_weights(cuda, strategy):
    import torch

    from dal import similarity as sim
    from dal import uncertainty_sampling as us
    from dal.engine import PoolState

    X, F, S, _ = case("vec4_binary")
    n, k = X.shape[0], 12
    lab, unl = np.arange(10), np.arange(10, n)
    state = PoolState(X, device=cuda)
    sel = us.select_batch(state, unl, lab, F, k, strategy=strategy, alpha=0.4)
    w_unl = _np(sel.weights)
    assert w_unl.dtype == np.float64 and w_unl.min() >= 0.0 and w_unl.max() <= 1.0
    if strategy != "entropy":  # one fp64 operation on an exact score
        assert w_unl.tobytes() == (1.0 - R.scores([S[i] for i in unl], 10, strategy)).tobytes()
    assert np.array_equal(_np(sel.sums), np.array([S[i] for i in unl], dtype=np.int64)) and sel.votes is None
    w = np.zeros(n)
    w[unl] = w_unl
    simx, _ = sim._bf16_pool(torch.from_numpy(np.array(X)).to(cuda), cuda)
    ref = sim.ranked_batch_select(simx, lab, torch.from_numpy(w).to(cuda), k, alpha=0.4, candidates=unl, device=cuda)
    assert np.array_equal(_np(sel.indices), _np(ref.indices)) and np.unique(_np(sel.indices)).size == k
    assert _np(sel.selected_scores).tobytes() == _np(ref.selected_scores).tobytes()
    assert _np(sel.selected_similarity).tobytes() == _np(ref.selected_similarity).tobytes()


def test_emulated_shards_equal_the_single_device(cuda):
    """Three shards of one device (512-row granule: the third holds 13 rows)
    merge to the single-device selection, for every strategy; every other mode
    refuses the forest."""
    from dal import parallel
    from dal import uncertainty_sampling as us

    X, F, S, flags = case("scalar_ragged")
    n, k = X.shape[0], 20
    unl = np.nonzero(flags)[0]
    for strategy in R.STRATEGIES:
        one = us.select(np.array(X), unl, F, k, strategy=strategy, device=cuda)
        for world in (2, 3):
            sels = []
            for r in range(world):
                lo, hi, _ = parallel.shard_range(n, world, r)
                sels.append(parallel.ShardedSelector(np.array(X[lo:hi]), n, r, world, device=cuda))
            idx, sc = parallel.emulate(sels, unl, F, k, mode="us", strategy=strategy)
            assert np.array_equal(_np(idx), _np(one.indices)), (strategy, world)
            assert _np(sc).tobytes() == _np(one.selected_scores).tobytes(), (strategy, world)
    with pytest.raises(ValueError, match="soft votes"):
        parallel.emulate(sels, unl, F, k, mode="dw")
    with pytest.raises(ValueError, match="soft votes"):
        sels[0].local_select(None, None, unl, F, k, mode="dw_multiclass")


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

        X, F, _, flags = case("scalar_ragged")
        n, k = X.shape[0], 20
        unl = np.nonzero(flags)[0]
        comm = parallel.TorchComm()
        out = {"backend": comm.backend}
        shard = parallel.ShardedSelector(torch.from_numpy(np.array(X)).to(dev), n, 0, 1, device=dev)
        for strategy in R.STRATEGIES:
            idx, sc = parallel.select(shard, comm, unl, F, k, mode="us", strategy=strategy)
            one = us.select(np.array(X), unl, F, k, strategy=strategy, device=dev)
            torch.cuda.synchronize()
            out[strategy] = (_np(idx), _np(sc), _np(one.indices), _np(one.selected_scores))
        q.put(out)
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
    for strategy in R.STRATEGIES:
        idx, sc, one_idx, one_sc = out[strategy]
        assert idx.shape[0] == 20 and np.array_equal(idx, one_idx), strategy
        assert sc.tobytes() == one_sc.tobytes(), strategy


def test_run_loop_soft_votes(cuda):
    """run_loop(soft_votes=True) over a 3-class pool, scikit-learn trainer: the
    history of the same loop with the restatement as select_fn."""
    from dal.loop import run_loop

    rng = np.random.default_rng(17)
    X = rng.random((400, 8)).astype(np.float32)
    y = (X[:, 0] * 3).astype(int).clip(0, 2) * 2 + 5

    def ref_select(strategy, pool, unlabeled, model, k):
        F = ProbabilityForest.from_sklearn(model)
        return R.select(R.sums(F, pool[unlabeled]), F.n_trees, "least_confidence", unlabeled, k)[0]

    kw = dict(strategy="uncertainty", window_size=20, n_estimators=10, max_iterations=3, seed=4, trainer="sklearn",
              soft_votes=True)
    got = run_loop(X, y, device=cuda, **kw)
    ref = run_loop(X, y, select_fn=ref_select, **kw)
    assert len(got.labeled_history) == 3
    for a, b in zip(got.labeled_history, ref.labeled_history):
        assert np.array_equal(np.asarray(a), np.asarray(b))
