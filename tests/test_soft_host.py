"""Soft-vote forests, host side: the ProbabilityForest builders against the
restatement (tests/soft_reference.py), the restatement against scikit-learn's
predict_proba, the builder's refusals, every host-side status of
dal_forest_score_soft, and the loop / sharded merge with the restatement
injected.  CPU only (no kernel launches)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import soft_reference as R
from dal import _lib, parallel
from dal.forest import Forest, ProbabilityForest, quantize_distribution

# (n, d, T, depth, C): the pools the definition was checked on
SKLEARN_SHAPES = [(1037, 30, 10, 4, 3), (2051, 64, 100, 6, 10), (600, 8, 255, 3, 2), (777, 20, 7, 5, 32)]


@functools.lru_cache(maxsize=None)
def sklearn_case(n, d, T, depth, C):
    """A seeded pool, a scikit-learn forest fitted on 300 of its rows with
    every class present, its ProbabilityForest and the restatement's sums."""
    from sklearn.ensemble import RandomForestClassifier

    rng = np.random.default_rng(1000 * C + d)
    X = rng.random((n, d)).astype(np.float32)
    y = (np.floor(X[:, 0] * C).astype(int) + (X[:, 1] > 0.6)) % C
    y[:C] = np.arange(C)  # every class among the fitted rows
    rf = RandomForestClassifier(n_estimators=T, max_depth=depth, random_state=0, n_jobs=1).fit(X[:300], y[:300])
    assert len(rf.classes_) == C
    F = ProbabilityForest.from_sklearn(rf)
    return X, rf, F, R.sums(F, X)


def test_from_sklearn_leaf_words_equal_the_restatement():
    X, rf, F, _ = sklearn_case(1037, 30, 10, 4, 3)
    assert F.n_trees == 10 and F.n_classes == 3 and F.depth <= 4 and np.array_equal(F.classes_, rf.classes_)
    assert F.inner.dtype == np.int32 and F.leaf_id.dtype == np.int32 and F.leaf_q.dtype == np.uint32
    assert F.inner.shape == (10, (1 << F.depth) - 1, 2) and F.leaf_id.shape == (10, 1 << F.depth)
    F.check()
    values = []
    for est in rf.estimators_:  # leaves in depth-first order, left first: the builder's numbering
        tr = est.tree_
        stack = [0]
        while stack:
            nd = stack.pop()
            if tr.children_left[nd] < 0:
                values.append(tr.value[nd, 0, :])
            else:
                stack += [tr.children_right[nd], tr.children_left[nd]]
    assert F.n_leaves == len(values) == sum(e.tree_.n_leaves for e in rf.estimators_)
    assert F.leaf_q.tolist() == R.quantize(values)
    assert int(F.leaf_q.max()) <= R.ONE
    # a leaf's row is the leaf scikit-learn's own apply() reaches, for every tree and row
    lr = R.leaf_rows(F, X)
    base = 0
    for t, est in enumerate(rf.estimators_):
        node = est.tree_.apply(X)
        q = np.array(R.quantize(est.tree_.value[node, 0, :]), dtype=np.uint32)
        assert np.array_equal(F.leaf_q[lr[t]], q)
        assert lr[t].min() >= base and lr[t].max() < base + est.tree_.n_leaves
        base += est.tree_.n_leaves


def _shallow_tree():
    # node 0: x[0] <= 0.5 -> node 1 (a leaf at level 1) else node 2: x[1] <= 0.25 -> leaf 3 else leaf 4
    feature = [0, -1, 1, -1, -1]
    threshold = [0.5, 0.0, 0.25, 0.0, 0.0]
    left = [1, -1, 3, -1, -1]
    right = [2, -1, 4, -1, -1]
    dist = [[0, 0, 0], [1, 1, 2], [0, 0, 0], [0, 5, 0], [3, 0, 1]]
    return feature, threshold, left, right, dist, [0]


def test_padding_repeats_a_shallow_leaf_id_over_its_subtree():
    F = ProbabilityForest.from_nodes(*_shallow_tree(), n_classes=3)
    assert F.depth == 2 and F.n_leaves == 3
    assert F.leaf_id.tolist() == [[0, 0, 1, 2]]
    assert F.inner[0, 1].tolist() == [0, int(np.array([np.inf], dtype=np.float32).view(np.int32)[0])]  # (0, +inf)
    assert F.leaf_q.tolist() == [[1 << 29, 1 << 29, 1 << 30], [0, 1 << 31, 0], [3 << 29, 0, 1 << 29]]
    X = np.array([[0.1, 0.9], [0.9, 0.1], [0.9, 0.9]], dtype=np.float32)
    assert R.sums(F, X) == F.leaf_q.tolist()
    assert F.hard().leaf.tolist() == [[2, 2, 1, 0]]


@pytest.mark.parametrize("shape", SKLEARN_SHAPES)
def test_hard_equals_the_arg_max_forest(shape):
    _, rf, F, _ = sklearn_case(*shape)
    H, G = F.hard(), Forest.from_sklearn(rf, multiclass=True)
    assert H.n_classes == G.n_classes and H.depth == G.depth and H.inner.tobytes() == G.inner.tobytes()
    q = F.leaf_q[F.leaf_id].astype(np.int64)  # [T, 2^D, C]
    top = np.sort(q, axis=2)
    unique = top[:, :, -1] > top[:, :, -2]
    assert unique.any()
    assert np.array_equal(H.leaf[unique], G.leaf[unique])


@pytest.mark.parametrize("shape", SKLEARN_SHAPES)
def test_probabilities_within_2_pow_minus_31_of_sklearn(shape):
    X, rf, F, S = sklearn_case(*shape)
    T = shape[2]
    p = R.proba(S, T)
    ref = rf.predict_proba(X)
    gap = np.abs(p - ref).max()
    print(f"{shape}: max |p - predict_proba| = {gap:.3e} (bound {2.0 ** -31:.3e})")
    assert gap <= 2.0 ** -31
    # the prediction is scikit-learn's wherever the largest sum is unique; where two classes hold the same exact
    # sum, scikit-learn's fp64 adds decide between them by rounding noise and the canonical choice is the lowest
    pred, ref_pred = R.pred(S), np.searchsorted(rf.classes_, rf.predict(X))
    tied = np.array([sorted(s)[-1] == sorted(s)[-2] for s in S])
    assert tied.mean() < 0.05 and np.array_equal(pred[~tied], ref_pred[~tied])
    for i in np.nonzero(tied)[0]:
        assert S[i][ref_pred[i]] == max(S[i]) and pred[i] <= ref_pred[i]


def test_soft_least_confidence_takes_more_than_T_plus_1_values():
    """What the feature is for: hard votes give at most T + 1 scores."""
    _, _, F, S = sklearn_case(1037, 30, 10, 4, 3)
    soft = R.scores(S, 10, "least_confidence")
    assert np.unique(soft).size > 10 + 1
    import multiclass_reference as MR

    X = sklearn_case(1037, 30, 10, 4, 3)[0]
    hard = MR.scores(MR.counts(F.hard(), X), 10, "least_confidence")
    assert np.unique(hard).size <= 11 < np.unique(soft).size


def test_synthetic_is_seeded_and_takes_one_hot_leaves():
    a = ProbabilityForest.synthetic(7, 3, 8, 5, seed=4)
    b = ProbabilityForest.synthetic(7, 3, 8, 5, seed=4, one_hot=[(2, 5, 3), (6, 0, 0)])
    a.check()
    assert a.leaf_id.tolist() == np.arange(56).reshape(7, 8).tolist() and a.n_leaves == 56
    assert a.inner.tobytes() == b.inner.tobytes() and a.hard().inner is a.inner
    assert b.leaf_q[2 * 8 + 5].tolist() == [0, 0, 0, R.ONE, 0] and b.leaf_q[6 * 8].tolist() == [R.ONE, 0, 0, 0, 0]
    rest = np.ones(56, dtype=bool)
    rest[[21, 48]] = False
    assert np.array_equal(a.leaf_q[rest], b.leaf_q[rest])
    assert (np.abs(a.leaf_q.astype(np.int64).sum(axis=1) - R.ONE) <= 5).all()


def test_builder_refusals():
    f, t, l, r, dist, roots = _shallow_tree()
    ok = np.array(dist, dtype=np.float64)

    def build(d=ok, n_classes=3, roots=roots):
        return ProbabilityForest.from_nodes(f, t, l, r, d, roots, n_classes=n_classes)

    build()
    for bad in (-1.0, float("nan"), float("inf")):
        d = ok.copy()
        d[3, 1] = bad
        with pytest.raises(ValueError):
            build(d)
    d = ok.copy()
    d[4] = 0.0  # an all-zero leaf row
    with pytest.raises(ValueError, match="all zero"):
        build(d)
    d = ok.copy()
    d[0] = -7.0  # (an inner node's row is never read)
    build(d)
    with pytest.raises(ValueError):
        build(ok[:, :2], n_classes=3)  # distribution narrower than n_classes
    with pytest.raises(ValueError, match="n_classes"):
        ProbabilityForest.from_nodes(f, t, l, r, np.ones((5, 1)), roots, n_classes=1)
    with pytest.raises(ValueError, match="n_classes"):
        ProbabilityForest.from_nodes(f, t, l, r, np.ones((5, 33)), roots, n_classes=33)
    with pytest.raises(ValueError, match="trees"):
        build(roots=[0] * 256)
    with pytest.raises(ValueError, match="no trees"):
        build(roots=[])
    # a chain one level deeper than the limit
    D = _lib.DAL_SOFT_MAX_DEPTH + 1
    feat = [0] * D + [-1] * (D + 1)
    left = list(range(1, D)) + [D] + [-1] * (D + 1)
    right = [D + 1 + i for i in range(D)] + [-1] * (D + 1)
    with pytest.raises(ValueError, match="DAL_SOFT_MAX_DEPTH"):
        ProbabilityForest.from_nodes(feat, [0.5] * (2 * D + 1), left, right, np.ones((2 * D + 1, 2)), [0], n_classes=2)
    with pytest.raises(ValueError):
        ProbabilityForest.synthetic(256, 3, 8, 3)
    with pytest.raises(ValueError):
        ProbabilityForest.synthetic(10, 3, 8, 33)
    with pytest.raises(ValueError):
        ProbabilityForest.synthetic(10, _lib.DAL_SOFT_MAX_DEPTH + 1, 8, 3)
    with pytest.raises(ValueError):
        quantize_distribution(np.zeros((0, 3)))


def test_refused_before_any_upload():
    """check() runs in device() before a tensor is made: a leaf id outside the
    table, too many trees and a feature outside the pool all raise on a
    machine without a GPU."""
    F = ProbabilityForest.synthetic(5, 3, 8, 4, seed=2)
    bad = ProbabilityForest(inner=F.inner, leaf_id=F.leaf_id.copy(), leaf_q=F.leaf_q, depth=3, n_classes=4)
    bad.leaf_id[1, 2] = F.n_leaves
    with pytest.raises(ValueError, match="leaf id"):
        bad.device("cuda:0")
    bad.leaf_id[1, 2] = -1
    with pytest.raises(ValueError, match="leaf id"):
        bad.device("cuda:0")
    wide = ProbabilityForest(inner=np.repeat(F.inner, 60, axis=0), leaf_id=np.repeat(F.leaf_id, 60, axis=0),
                             leaf_q=F.leaf_q, depth=3, n_classes=4)
    with pytest.raises(ValueError, match="trees"):
        wide.device("cuda:0")
    with pytest.raises(ValueError, match="outside the pool"):
        F.check_features(int(F.inner[..., 0].max()))
    F.check_features(8)


def test_abi_statuses_without_gpu():
    lib = _lib.load()
    assert lib.dal_abi_version() == 10
    limit = lib.dal_forest_soft_max_depth()
    assert limit == _lib.DAL_SOFT_MAX_DEPTH >= 12
    p = ctypes.c_void_p(256)
    ARG, SHAPE, UNSUPPORTED = -1, -2, -3

    def score(x=p, n=10, d=4, x_stride=4, inner=p, leaf_id=p, leaf_q=p, L=20, T=10, depth=4, C=3, kind=0, flags=None,
              order=0, sums=p, pred=p, scores=p, keys=p):
        return lib.dal_forest_score_soft(x, n, d, x_stride, inner, leaf_id, leaf_q, L, T, depth, C, kind, flags, order,
                                         sums, pred, scores, keys, None)

    for name in ("x", "inner", "leaf_id", "leaf_q", "scores", "keys"):
        assert score(**{name: None}) == ARG, name
    assert score(kind=3) == ARG and score(kind=-1) == ARG and score(order=2) == ARG and score(order=-1) == ARG
    assert score(x_stride=3) == SHAPE and score(d=30, x_stride=29) == SHAPE and score(d=30, x_stride=0) == SHAPE
    assert score(n=-1) == SHAPE and score(d=0, x_stride=0) == SHAPE and score(L=0) == SHAPE
    assert score(T=256) == UNSUPPORTED and score(T=0) == UNSUPPORTED
    assert score(C=33) == UNSUPPORTED and score(C=1) == UNSUPPORTED
    assert score(depth=limit + 1) == UNSUPPORTED and score(depth=0) == UNSUPPORTED
    # the documented order: ARG before SHAPE before UNSUPPORTED
    assert score(x=None, x_stride=3) == ARG
    assert score(x=None, x_stride=3, T=256) == ARG
    assert score(x_stride=3, T=256) == SHAPE and score(x_stride=3, C=33, depth=limit + 1) == SHAPE
    # nothing to score: no launch; sums and pred are optional; the limits themselves pass
    assert score(n=0) == 0 and score(n=0, sums=None, pred=None) == 0
    assert score(n=0, T=255, C=32, depth=limit) == 0 and score(n=0, T=1, C=2, depth=1, d=1, x_stride=1) == 0
    assert score(n=0, x_stride=7) == 0  # any stride >= d


# ------------------------------------------------- the loop and the merge --
def _restatement_select(strategy_name):
    def select_fn(strategy, pool, unlabeled, model, k):
        F = ProbabilityForest.from_sklearn(model)
        return R.select(R.sums(F, pool[unlabeled]), F.n_trees, strategy_name, unlabeled, k)[0]
    return select_fn


def test_run_loop_soft_votes_arguments_and_restatement():
    from dal.loop import run_loop

    rng = np.random.default_rng(3)
    X = rng.random((240, 6)).astype(np.float32)
    y = (X[:, 0] * 3).astype(int).clip(0, 2)
    for strategy in ("density", "information_density", "lal", "random"):
        with pytest.raises(ValueError, match="soft_votes"):
            run_loop(X, y, strategy=strategy, trainer="sklearn", soft_votes=True, max_iterations=1)
    with pytest.raises(ValueError, match="trainer='gpu'"):
        run_loop(X, y, strategy="uncertainty", soft_votes=True, num_classes=3, max_iterations=1)
    kw = dict(strategy="uncertainty", window_size=20, n_estimators=10, max_iterations=3, seed=4, trainer="sklearn",
              select_fn=_restatement_select("least_confidence"))
    a, b = run_loop(X, y, soft_votes=True, **kw), run_loop(X, y, **kw)
    assert len(a.labeled_history) == 3
    for u, v in zip(a.labeled_history, b.labeled_history):  # (select_fn replaces the step: the flag only validates)
        assert np.array_equal(u, v)
    picked = np.concatenate(a.labeled_history)
    assert np.unique(picked).size == 60 and picked.min() >= 20


class _HostState:
    """What ShardedSelector.status_word reads of a shard's PoolState."""

    status = torch.zeros(1, dtype=torch.int32)


class RestatementShard(parallel.ShardedSelector):
    """ShardedSelector whose local step is the restatement (CPU)."""

    def __init__(self, X, n_total, rank, world):
        self.n_total, self.rank, self.world = n_total, rank, world
        self.lo, self.hi, self.shard = parallel.shard_range(n_total, world, rank)
        self.x = X[self.lo:self.hi]
        self.state = _HostState()
        self._density = None

    def index_tensor(self, unl):
        return torch.as_tensor(np.asarray(unl), dtype=torch.int64)

    def local_select(self, u_full, parts_full, unl, forest, k, mode="dw", strategy="least_confidence", beta=1.0,
                     density_mode="gram", warm=None):
        parallel._soft_forest(forest, mode)
        keys = torch.full((k,), parallel._as_i64(R.KEY_NONE), dtype=torch.int64)
        idx = torch.full((k,), -1, dtype=torch.int64)
        sc = torch.full((k,), float("nan"), dtype=torch.float64)
        unl = np.asarray(unl)
        mine = unl[(unl >= self.lo) & (unl < self.hi)]
        if mine.size:
            si, ss = R.select(R.sums(forest, self.x[mine - self.lo]), forest.n_trees, strategy, mine, k)
            kk = si.size
            ky = R.keys(ss, np.ones(kk, dtype=np.uint8), R.ASCENDING[strategy])
            keys[:kk] = torch.from_numpy(ky.view(np.int64))
            idx[:kk] = torch.from_numpy(si)
            sc[:kk] = torch.from_numpy(ss)
        return parallel.LocalTopk(keys, idx, sc)


def _cpu_sort_positions(keys, pos, k):
    order = np.lexsort((pos.numpy(), keys.numpy().view(np.uint64)))[:k]
    return torch.from_numpy(order.astype(np.int64))


@pytest.mark.parametrize("strategy", R.STRATEGIES)
def test_emulate_merge_equals_the_single_selection(strategy):
    """1, 2, 3 and 5 shards of 1,037 rows (512-row granule: at 5 shards the
    last two hold no row at all), and a rank whose rows are all labeled."""
    n, d, k = 1037, 30, 25
    X, _, F, S = sklearn_case(1037, 30, 10, 4, 3)
    unl = np.arange(7, n)
    unl = unl[(unl < 512) | (unl >= 1024)]  # (at 3 shards rank 1 holds rows and no candidate)
    ref_idx, ref_sc = R.select([S[i] for i in unl], 10, strategy, unl, k)
    for world in (1, 2, 3, 5):
        sels = [RestatementShard(X, n, r, world) for r in range(world)]
        if world == 5:
            assert sum(s.hi == s.lo for s in sels) >= 1
        idx, sc = parallel.emulate(sels, unl, F, k, mode="us", strategy=strategy, sort_fn=_cpu_sort_positions)
        assert np.array_equal(idx.numpy(), ref_idx), (strategy, world)
        assert np.array_equal(sc.numpy(), ref_sc), (strategy, world)
    # fewer candidates than k: the padding keys never reach the result
    few = unl[:9]
    idx, sc = parallel.emulate([RestatementShard(X, n, r, 3) for r in range(3)], few, F, k, mode="us",
                               strategy=strategy, sort_fn=_cpu_sort_positions)
    ref_idx, ref_sc = R.select([S[i] for i in few], 10, strategy, few, k)
    assert idx.shape[0] == 9 and np.array_equal(idx.numpy(), ref_idx) and np.array_equal(sc.numpy(), ref_sc)


@pytest.mark.parametrize("mode", ["dw", "dw_multiclass"])
def test_every_other_sharded_mode_refuses_a_soft_forest(mode):
    X, _, F, _ = sklearn_case(1037, 30, 10, 4, 3)
    sels = [RestatementShard(X, 1037, r, 2) for r in range(2)]
    with pytest.raises(ValueError, match="soft votes"):
        parallel.emulate(sels, np.arange(10, 1037), F, 5, mode=mode, sort_fn=_cpu_sort_positions)
    with pytest.raises(ValueError, match="soft votes"):
        parallel.select(sels[0], None, np.arange(10, 1037), F, 5, mode=mode)
    with pytest.raises(ValueError, match="soft votes"):
        parallel.ShardedSelector.local_select(sels[0], None, None, np.arange(10, 1037), F, 5, mode=mode)
