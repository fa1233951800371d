"""GPU training of regression forests (dal_rf_train_regressor,
csrc/rf_train_regress.hip) against the restatement on Python integers
(tests/rf_regress_reference.py).

Both sides take the same bagging draws.  The variance sums are exact on both
sides and every statistic is rounded once, so the heap arrays
(inner_feature, inner_threshold, leaf) and the per-feature thresholds must be
equal byte for byte -- whatever order the atomics arrive in."""
import functools

import numpy as np
import pytest

import lal_reference as L
import rf_regress_reference as G
from conftest import load_golden

pytestmark = pytest.mark.gpu

# name: (seed index, n, d, T, depth)
CASES = {
    "smooth": (0, 300, 5, 6, 4),     # sin(6 x0) + x1 / 2 + noise
    "decades": (1, 300, 5, 6, 4),    # +-10^e (1 + x0), e in -8..3: the widest accumulators
    "offset": (2, 300, 5, 4, 4),     # 1e8 + small: the structure depends on the summation order
    "ints": (3, 200, 4, 4, 3),       # integer labels: impurity exactly 0.0 presets leaves
    "tiny": (4, 48, 3, 3, 2),        # fewer rows than bins
    "one_tree": (5, 300, 5, 1, 4),   # m = d, unit weights
    "deep": (6, 400, 5, 3, 6),       # levels 0-4 in LDS, level 5 past the 64 KiB budget: global atomics
    "blocks": (7, 2500, 4, 2, 3),    # three histogram blocks flush into one cell
    "f64": (8, 300, 5, 4, 4),        # fp64 rows v / T and a square root: not fp32-representable
}


@functools.lru_cache(maxsize=None)
def _data(name):
    from dal.random_forest import bagging_inputs, regression_subset_strategy

    i, n, d, T, depth = CASES[name]
    rng = np.random.default_rng(300 + i)
    X = rng.random((n, d), dtype=np.float32)
    x0 = X[:, 0].astype(np.float64)
    if name == "decades":
        y = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.integers(-8, 4, n) * (1.0 + x0)
    elif name == "offset":
        y = 1e8 + np.floor(4 * x0) * 1e-3 + 1e-4 * rng.random(n)
    elif name == "ints":
        y = np.floor(3 * x0)
    elif name == "f64":
        v = rng.integers(0, 51, n)
        X = rng.random((n, d))
        X[:, 0] = v / 50.0
        X[:, 1] = np.sqrt(v / 50.0 * (1.0 - v / 50.0) * 50.0 / 49.0)
        assert not np.array_equal(X[:, :2], X[:, :2].astype(np.float32).astype(np.float64))
        y = np.sin(6 * X[:, 0]) + X[:, 1] / 2 + 0.05 * rng.standard_normal(n)
    else:
        y = np.sin(6 * x0) + X[:, 1].astype(np.float64) / 2 + 0.05 * rng.standard_normal(n)
    w, s = bagging_inputs(n, d, T, depth, seed=T + depth, feature_subset_strategy=regression_subset_strategy(T))
    assert s.shape[2] == G.subset_size(d, T)
    return X, y, w, s, T, depth


@functools.lru_cache(maxsize=None)
def _reference(name):
    X, y, w, s, T, depth = _data(name)
    return G.train_regressor(X, y, w, s, max_depth=depth)


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(model, thr, arrays):
    feat, t, leaf = arrays
    assert _same_bytes(model.inner_feature, feat)
    assert _same_bytes(model.inner_threshold, t)
    assert _same_bytes(model.leaf, leaf)
    t_dev, ns_dev = (a.cpu().numpy() for a in model.split_thresholds)
    assert t_dev.dtype == np.float64
    for f, tf in enumerate(thr):
        assert ns_dev[f] == tf.size
        assert _same_bytes(t_dev[f, :tf.size], tf)


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_train_matches_reference(cuda, name):
    from dal.random_forest import check_regression_labels, train_regressor

    X, y, w, s, T, depth = _data(name)
    thr, sf, arrays = _reference(name)
    splits = (sf >= 0).sum(axis=1)
    if name == "smooth":
        assert (splits >= 9).all(), splits              # the trees are real trees
    assert (splits >= 2).all(), splits
    _, (_, ky), (_, kq) = check_regression_labels(y, X.shape[0])
    if name == "decades":
        assert ky >= 3 and kq >= 5                      # the widest accumulators of the set
    if name == "ints":
        # a pure child is a leaf above the last level
        assert any(sf[t, h] < 0 <= sf[t, (h - 1) // 2] for t in range(T) for h in range(1, sf.shape[1]))
    if name == "deep":
        # 1 + ky + kq words x 33 bins x 2 slots: level 4 fits the 64 KiB LDS budget, level 5 does not
        cell = (1 + ky + kq) * 8
        assert 16 * (2 * 33 + 1) * cell <= 65536 < 32 * (2 * 33 + 1) * cell
        assert (sf[:, 31:] >= 0).any()                  # level 5 really splits
    model = train_regressor(X, y, T, max_depth=depth, weights=w, feature_subsets=s, device=cuda)
    assert model.depth == depth and model.n_trees == T
    _check(model, thr, arrays)


@pytest.mark.parametrize("case", ["min_instances", "min_gain", "bins4", "bins100", "depth1", "constant_features",
                                  "constant_labels", "constant_labels_inexact", "heavy_weights", "negative_labels"])
def test_gpu_train_edge_cases_match_reference(cuda, case):
    """MLlib's strategy knobs and degenerate inputs on smooth's data."""
    from dal.random_forest import bagging_inputs, regression_subset_strategy, train_regressor

    X, y, w, s, T, depth = _data("smooth")
    kw, rkw, max_bins = {}, {}, 32
    if case == "min_instances":
        kw, rkw = dict(min_instances_per_node=25), dict(min_instances=25)
    elif case == "min_gain":
        kw, rkw = dict(min_info_gain=0.01), dict(min_info_gain=0.01)
    elif case == "bins4":
        max_bins = 4
    elif case == "bins100":
        max_bins = 100
    elif case == "depth1":
        depth = 1
        w, s = bagging_inputs(X.shape[0], X.shape[1], T, depth, seed=T + depth,
                              feature_subset_strategy=regression_subset_strategy(T))
    elif case == "constant_features":
        X = X.copy()
        X[:, 0] = 0.5
        X[:, 3] = -2.0
    elif case == "constant_labels":
        y = np.full(X.shape[0], 2.75)       # sums exact in fp64: impurity exactly 0.0
    elif case == "constant_labels_inexact":
        y = np.full(X.shape[0], 0.1)        # rounded sums: whatever the restatement grows
    elif case == "heavy_weights":
        w = (w * 37).astype(np.int32)
    elif case == "negative_labels":
        y = -np.abs(y) - 0.25
    model = train_regressor(X, y, T, max_depth=depth, max_bins=max_bins, weights=w, feature_subsets=s, device=cuda,
                            **kw)
    thr, sf, arrays = G.train_regressor(X, y, w, s, max_depth=depth, max_bins=max_bins, **rkw)
    _check(model, thr, arrays)
    if case == "constant_labels":
        assert (sf < 0).all() and (model.leaf == 2.75).all()    # a root leaf equal to y exactly
    if case == "negative_labels":
        assert (model.leaf < 0).all()
    if case in ("min_instances", "min_gain"):
        assert not np.array_equal(sf, _reference("smooth")[1])  # the knob changes the trees


def test_repeated_fit_and_chunks_are_identical(cuda):
    from dal.random_forest import train_regressor

    for name in ("offset", "deep"):
        X, y, w, s, T, depth = _data(name)
        fit = lambda **kw: train_regressor(X, y, T, max_depth=depth, weights=w, feature_subsets=s,  # noqa: E731
                                           device=cuda, **kw)
        a, b, c = fit(), fit(), fit(tree_chunk=T - 1)
        for m in (b, c):
            assert _same_bytes(a.inner_feature, m.inner_feature)
            assert _same_bytes(a.inner_threshold, m.inner_threshold)
            assert _same_bytes(a.leaf, m.leaf)
        _check(c, *_reference(name)[::2])


def test_trained_forest_predicts_like_the_reference(cuda):
    from dal.random_forest import predict_regression, train_regressor

    for name in ("smooth", "f64"):
        X, y, w, s, T, depth = _data(name)
        _, _, arrays = _reference(name)
        model = train_regressor(X, y, T, max_depth=depth, weights=w, feature_subsets=s, device=cuda)
        Xq = np.random.default_rng(9).random((700, X.shape[1])).astype(X.dtype)
        want = L.regress(G.heap_forest(arrays), Xq)
        assert L.bits_equal(predict_regression(model, Xq, device=cuda).cpu().numpy(), want)
        own = predict_regression(model, X, device=cuda).cpu().numpy()
        assert np.mean((own - y) ** 2) < 0.5 * np.var(y)        # it fits its training set


@functools.lru_cache(maxsize=None)
def _lal_table():
    """A seeded 400 x 9 table in the layout of the reference's regression
    data: the five LAL features in columns 0, 1, 2, 5, 7, the label last."""
    rng = np.random.default_rng(41)
    n, Tc = 400, 10
    t = rng.random((n, 9))
    v = rng.integers(0, Tc + 1, n)
    t[:, 0] = v / float(Tc)
    t[:, 1] = np.sqrt((v * (1 - v / Tc) ** 2 + (Tc - v) * (v / Tc) ** 2) / (Tc - 1))
    t[:, 5] = 0.1 + 0.4 * rng.random(n)
    t[:, 7] = rng.integers(10, 41, n)
    t[:, 8] = 0.3 * t[:, 1] - 0.1 * np.abs(t[:, 0] - 0.5) + 0.2 * t[:, 5] - 0.002 * t[:, 7] \
        + 0.02 * rng.standard_normal(n)
    return t


@functools.lru_cache(maxsize=None)
def _lal_reference(T=20, seed=3):
    from dal.random_forest import bagging_inputs

    t = _lal_table()
    X, y = t[:, [0, 1, 2, 5, 7]], t[:, -1]
    w, s = bagging_inputs(400, 5, T, 4, seed, "onethird")
    assert s.shape[2] == 2
    return G.train_regressor(X, y, w, s, max_depth=4)


def test_train_lal_model_matches_reference(cuda, tmp_path):
    from dal.active_learner import train_lal_model

    thr, sf, arrays = _lal_reference()
    assert ((sf >= 0).sum(axis=1) >= 5).all()
    used = set(sf[sf >= 0].tolist())
    assert used >= {0, 1, 3, 4}                                 # the features drive the splits
    model = train_lal_model(_lal_table(), num_trees=20, seed=3, device=cuda)
    _check(model, thr, arrays)
    p = tmp_path / "reg.txt"
    p.write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in _lal_table()) + "\n")
    _check(train_lal_model(str(p), num_trees=20, seed=3, device=cuda), thr, arrays)


def test_lal_loop_with_the_trained_model(cuda):
    from dal import loop
    from dal.active_learner import train_lal_model

    g = load_golden("checkerboard2x2.npz")
    X, y = g["X"][:300], g["y"][:300]
    assert X.shape[0] == 300
    trained = train_lal_model(_lal_table(), num_trees=20, seed=3, device=cuda)
    reference = G.heap_forest(_lal_reference()[2])
    kw = dict(strategy="lal", trainer="gpu", max_iterations=3, window_size=10, device=cuda)
    got = loop.run_loop(X, y, X, y, lal_model=trained, **kw)
    ref = loop.run_loop(X, y, X, y, lal_model=reference, **kw)
    assert got.log == ref.log and len(got.labeled_history) == 3
    for a, b in zip(got.labeled_history, ref.labeled_history):
        assert np.array_equal(a, b)
