"""Multiclass uncertainty sampling on the GPU: dal_forest_score_multiclass
(per-class counts, prediction, score, key) and everything above it, bit-exact
against the NumPy restatement of the canonical semantics
(tests/multiclass_reference.py)."""
import functools

import numpy as np
import pytest

import multiclass_reference as R
from dal import _lib
from dal.forest import Forest
from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu

KEY_NONE = np.uint64(_lib.DAL_KEY_NONE)


def _flags(n, seed):
    """~70 % of the rows marked DAL_ROW_CANDIDATE (seeded)."""
    return (np.random.default_rng(seed).random(n) < 0.7).astype(np.uint8)


def _score(cuda, state, F, strategy, flags):
    """One launch through the engine; numpy (counts, pred, scores, keys)."""
    import torch

    from dal import engine

    fl = None if flags is None else torch.from_numpy(flags).to(cuda)
    order = _lib.DAL_ASCENDING if R.ASCENDING[strategy] else _lib.DAL_DESCENDING
    lut = engine.device_multiclass_lut(strategy, F.n_trees, cuda)
    c, p, s, k = engine.forest_score_multiclass(state, F, lut, fl, order, engine.MULTICLASS_KINDS[strategy])
    return c.cpu().numpy(), p.cpu().numpy(), s.cpu().numpy(), k.cpu().numpy().view(np.uint64)


def _check_all(cuda, X, F, seed=11):
    """Every strategy over one pool: counts, pred and scores equal the
    reference, keys are DAL_KEY_NONE exactly on the rows that are no candidates."""
    from dal.engine import PoolState

    cnt = R.counts(F, X)
    assert (cnt.sum(axis=1) == F.n_trees).all()
    state = PoolState(X, device=cuda)
    flags = _flags(X.shape[0], seed)
    for strategy in R.STRATEGIES:
        c, p, s, k = _score(cuda, state, F, strategy, flags)
        assert c.shape == cnt.shape and c.dtype == np.uint8
        assert np.array_equal(c, cnt), strategy
        assert np.array_equal(p, R.pred(cnt)), strategy
        ref = R.scores(cnt, F.n_trees, strategy)
        assert np.array_equal(s, ref) and not np.signbit(s[s == 0.0]).any(), strategy
        assert np.array_equal(k == KEY_NONE, flags == 0), strategy
    return cnt


# (n, d, T, depth, C): the smallest shape of each launcher path
SHAPES = [
    (1037, 30, 10, 4, 3),
    (1037, 13, 10, 4, 3),
    (3001, 64, 100, 4, 10),
    (2500, 256, 10, 4, 10),
    (700, 1100, 10, 3, 4),
    (600, 40, 255, 8, 32),
    (65, 1, 1, 1, 2),
]


@pytest.mark.parametrize("n,d,T,depth,C", SHAPES)
def test_shapes(cuda, n, d, T, depth, C):
    """The launcher's paths (its thresholds are the binary row-major kernel's):
    1,037 x 30   scalar staging (d % 4 != 0), 128-row tiles, tpr 2, ragged last block, C % 4 != 0, CW 1
    1,037 x 13   scalar staging, 256-row tiles, tpr 1 (30 features no longer fit 256 rows in 16 KiB), ragged
    3,001 x 64   16-byte staging, 64-row tiles, tpr 4 (T >= 64), CW 4, 16-bit count stores
    2,500 x 256  LDS-DMA, 32-row tiles, tpr 8, persistent grid
    700 x 1,100  rows from global memory (16 rows pass 64 KiB), tpr 1, CW 1, 32-bit count stores
    600 x 40     forest from global memory (585 KB), CW 8, T at the limit, tpr 4
    65 x 1       minimal: one tree, one level, two classes, one feature"""
    X = O.synthetic_pool(n, d, seed=n % 97)
    F = Forest.synthetic(T, depth, d, seed=5, n_classes=C)
    _check_all(cuda, X, F)


def test_dma_block_walks_two_tiles(cuda):
    """LDS-DMA at d = 128 (64-row tiles) with more tiles than twice the
    resident grid: a block's LDS (rows, LUT, forest) bounds the blocks per CU,
    so n = 2 x CUs x that bound x 64 rows (+ a ragged tile) makes every block
    of the persistent grid walk at least two tiles."""
    import torch

    d, T, depth, C, rows = 128, 10, 4, 10, 64
    lds = rows * (d + 4) * 4 + (T + 2) * 8 + T * (((1 << depth) - 1) * 8 + (1 << depth))
    per_cu = (160 * 1024) // lds
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    n = min(2 * cus * per_cu * rows + 37, 400_000)
    assert n > cus * per_cu * rows  # the second tile of at least one block, whatever the cap
    X = O.synthetic_pool(n, d, seed=3)
    F = Forest.synthetic(T, depth, d, seed=6, n_classes=C)
    _check_all(cuda, X, F)


def _constant_leaf_forest(T, depth, d, C, tree_class):
    F = Forest.synthetic(T, depth, d, seed=9, n_classes=C)
    leaf = np.empty_like(F.leaf)
    leaf[:] = np.asarray(tree_class, dtype=np.uint8)[:, None]
    return Forest(inner=F.inner, leaf=leaf, depth=depth, n_classes=C)


def test_counter_field_saturates_at_255(cuda):
    """Every tree votes class 3 of 5: one field reaches 255, its neighbours stay 0."""
    X = O.synthetic_pool(3000, 64, seed=1)
    F = _constant_leaf_forest(255, 3, 64, 5, [3] * 255)
    cnt = _check_all(cuda, X, F)
    assert (cnt[:, 3] == 255).all() and (np.delete(cnt, 3, axis=1) == 0).all()


def test_adjacent_counter_fields_across_the_lane_sum(cuda):
    """128 trees of class 4 and 127 of class 5, C = 8: adjacent fields of one
    word, each summed over the row's lanes (tpr 4 at T >= 64)."""
    X = O.synthetic_pool(3000, 64, seed=2)
    F = _constant_leaf_forest(255, 3, 64, 8, [4] * 128 + [5] * 127)
    cnt = _check_all(cuda, X, F)
    assert (cnt[:, 4] == 128).all() and (cnt[:, 5] == 127).all() and cnt.sum() == 255 * 3000


def test_skewed_forest_large_counts(cuda):
    X = O.synthetic_pool(3000, 40, seed=4)
    F = Forest.synthetic(255, 4, 40, seed=8, n_classes=32, skew=0.97)
    assert R.counts(F, X).max() >= 240  # (on the CPU first: the inputs cannot go soft)
    _check_all(cuda, X, F)


@pytest.mark.parametrize("n,d,T,depth,C", SHAPES[:-1])
def test_selection(cuda, n, d, T, depth, C):
    """us.select against the reference at every multiclass shape (the
    two-class one routes to the binary kernels): k = 1 and 100, an unlabeled
    subset, and k above the candidate count (clamped).  Least confidence and
    margin take a handful of values, so the k-th boundary is a tie broken by
    the index."""
    from dal import uncertainty_sampling as us
    from dal.engine import PoolState

    X = O.synthetic_pool(n, d, seed=21)
    F = Forest.synthetic(T, depth, d, seed=7, n_classes=C)
    cnt = R.counts(F, X)
    state = PoolState(X, device=cuda)
    rng = np.random.default_rng(n)
    subset = np.sort(rng.choice(n, size=(2 * n) // 3, replace=False))
    few = np.sort(rng.choice(n, size=40, replace=False))
    for strategy in R.STRATEGIES:
        for unl, k in ((np.arange(n), 1), (np.arange(n), 100), (subset, 100), (few, 100)):
            sel = us.select(state, unl, F, k, strategy=strategy)
            ref_idx, ref_sc = R.select(cnt[unl], T, strategy, unl, k)
            assert ref_idx.shape[0] == min(k, unl.shape[0])
            assert np.array_equal(sel.indices.cpu().numpy(), ref_idx), (strategy, k)
            assert np.array_equal(sel.selected_scores.cpu().numpy(), ref_sc), (strategy, k)
            assert sel.votes is None
            assert np.array_equal(sel.counts.cpu().numpy(), cnt[unl])
            assert np.array_equal(sel.scores.cpu().numpy(), R.scores(cnt[unl], T, strategy))


def test_two_classes_match_the_binary_votes(cuda):
    """On a binary forest the multiclass kernel's counts[:, 1] are
    dal_forest_score's votes, bit for bit."""
    from dal import engine

    X = O.synthetic_pool(3001, 64, seed=12)
    F = Forest.synthetic(100, 4, 64, seed=3)
    state = engine.PoolState(X, device=cuda)
    lut = engine.device_lut("least_confidence", F.n_trees, cuda)
    votes, _, _, _ = engine.forest_score(state, F, lut, state.flags, _lib.DAL_ASCENDING)
    c, p, _, _ = _score(cuda, state, F, "least_confidence", None)
    votes = votes.cpu().numpy()
    assert np.array_equal(c[:, 1].astype(np.int32), votes) and np.array_equal(c[:, 0], 100 - votes)
    assert np.array_equal(p, (2 * votes > 100).astype(np.uint8))  # ties -> class 0, as the binary predict


@functools.lru_cache(maxsize=None)
def _sklearn_case(name, max_depth):
    from sklearn import datasets
    from sklearn.ensemble import RandomForestClassifier

    data = datasets.load_iris() if name == "iris" else datasets.load_digits()
    X = data.data.astype(np.float32)
    y = data.target * 3 + 1  # labels need not be contiguous
    rf = RandomForestClassifier(n_estimators=20, max_depth=max_depth, random_state=0).fit(X, y)
    return X, rf


@pytest.mark.parametrize("name", ["iris", "digits"])
@pytest.mark.parametrize("max_depth", [4, 8])
def test_sklearn_hard_votes(cuda, name, max_depth):
    """counts equal the trees' own hard votes (est.predict gives the class
    index; classes_ maps it to the label) -- not rf.predict, which averages
    probabilities."""
    from dal import random_forest

    X, rf = _sklearn_case(name, max_depth)
    F = Forest.from_sklearn(rf, multiclass=True)
    assert np.array_equal(F.classes_, rf.classes_) and F.n_classes == len(rf.classes_)
    hard = np.stack([e.predict(X) for e in rf.estimators_]).astype(int)
    labels = rf.classes_[hard]  # [T, n] labels voted
    ref = np.stack([(labels == lab).sum(axis=0) for lab in F.classes_], axis=1)
    pred, counts = random_forest.predict(F, X, device=cuda)
    assert np.array_equal(counts.cpu().numpy(), ref)
    assert np.array_equal(pred.cpu().numpy(), np.argmax(ref, axis=1))
    _check_all(cuda, X, F)


def test_sharded_selection_equals_single_gpu(cuda):
    from dal import parallel
    from dal import uncertainty_sampling as us

    n, d, world, k = 10_007, 24, 3, 50
    X = O.synthetic_pool(n, d, seed=31)
    F = Forest.synthetic(10, 4, d, seed=2, n_classes=10)
    unl = np.arange(17, n)
    sels = []
    for r in range(world):
        lo, hi, _ = parallel.shard_range(n, world, r)
        sels.append(parallel.ShardedSelector(X[lo:hi], n, r, world, device=cuda))
    assert len({s.hi - s.lo for s in sels}) > 1  # uneven shards
    cnt = R.counts(F, X)
    for strategy in R.STRATEGIES:
        idx, sc = parallel.emulate(sels, unl, F, k, mode="us", strategy=strategy)
        one = us.select(X, unl, F, k, strategy=strategy, device=cuda)
        assert np.array_equal(idx.cpu().numpy(), one.indices.cpu().numpy())
        assert np.array_equal(sc.cpu().numpy(), one.selected_scores.cpu().numpy())
        ref_idx, ref_sc = R.select(cnt[unl], 10, strategy, unl, k)
        assert np.array_equal(idx.cpu().numpy(), ref_idx) and np.array_equal(sc.cpu().numpy(), ref_sc)
    with pytest.raises(ValueError, match="binary only"):
        sels[0].local_select(None, None, unl, F, k, mode="dw")


def test_run_loop_three_classes(cuda):
    """run_loop over a seeded 3-class pool, scikit-learn trainer, 3 iterations:
    the history equals the same loop with the reference as select_fn."""
    from dal.loop import run_loop

    rng = np.random.default_rng(17)
    X = rng.random((600, 8)).astype(np.float32)
    y = (X[:, 0] * 3).astype(int).clip(0, 2) * 2 + 5  # labels 5, 7, 9
    assert len(set(y[:20].tolist())) == 3  # every class in the initial window: each forest has 3 classes

    def ref_select(strategy, pool, unlabeled, model, k):
        F = Forest.from_sklearn(model, multiclass=True)
        assert F.n_classes == 3
        return R.select(R.counts(F, pool[unlabeled]), F.n_trees, "least_confidence", unlabeled, k)[0]

    kw = dict(strategy="uncertainty", window_size=20, n_estimators=10, max_iterations=3, seed=4, trainer="sklearn")
    got = run_loop(X, y, device=cuda, **kw)
    ref = run_loop(X, y, select_fn=ref_select, **kw)
    assert len(got.labeled_history) == 3
    for a, b in zip(got.labeled_history, ref.labeled_history):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_predict_ties_go_to_the_lowest_class(cuda):
    from dal import random_forest

    X = O.synthetic_pool(300, 6, seed=5)
    F = _constant_leaf_forest(4, 1, 6, 5, [3, 1, 3, 1])  # classes 1 and 3 tie at two trees each
    pred, counts = random_forest.predict(F, X, device=cuda)
    assert (counts.cpu().numpy() == np.array([0, 2, 0, 2, 0], dtype=np.uint8)).all()
    assert (pred.cpu().numpy() == 1).all()
    G = _constant_leaf_forest(3, 1, 6, 4, [2, 0, 3])  # a three-way tie at one tree each
    pred, _ = random_forest.predict(G, X, device=cuda)
    assert (pred.cpu().numpy() == 0).all()
