"""GPU forest training for C classes (dal_rf_train_multiclass,
csrc/rf_train_multi.hip) against the NumPy restatement of MLlib 2.1's
trainClassifier(numClasses=C) (tests/rf_multiclass_reference.py).

Both sides take the same bagging_inputs draws; the heap arrays (inner, leaf)
and the per-feature thresholds must then match bit for bit: histograms are
integer sums, the Gini gain is fp64 in one fixed operation order on both
sides, and ties go to the first maximum."""
import functools

import numpy as np
import pytest

import multiclass_dw_reference as DW
import multiclass_reference as R
import rf_multiclass_reference as M
from conftest import load_golden
from dal.forest import Forest
from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu

# name: (seed index, n, d, C, T, depth)
CASES = {
    "c3": (0, 300, 8, 3, 10, 4),             # the common case
    "c10": (1, 700, 12, 10, 7, 4),
    "c32_deep": (2, 400, 6, 32, 5, 6),       # levels 0-2: LDS histogram (<= 64 KiB); 3-5: global atomics
    "c5_tiny": (3, 64, 4, 5, 3, 2),          # few rows, few bins
    "c32_one_tree": (4, 500, 6, 32, 1, 4),   # one tree: all features, unit weights, m = d
    "c4_absent": (5, 300, 8, 4, 10, 4),      # class 1 relabelled to 3: a zero count in every node
    "c3_int": (6, 400, 5, 3, 10, 4),         # integer features 0..3: fewer distinct values than splits
}


@functools.lru_cache(maxsize=None)
def _data(name):
    from dal.random_forest import bagging_inputs

    i, n, d, C, T, depth = CASES[name]
    rng = np.random.default_rng(100 + i)
    if name == "c3_int":
        X = rng.integers(0, 4, (n, d)).astype(np.float32)
        y = (X[:, 0] + X[:, 1]).astype(np.int64) % 3
    else:
        X = rng.random((n, d), dtype=np.float32)
        y = np.minimum(np.floor(X[:, 0] * C).astype(np.int64) + (X[:, 1] > 0.8), C - 1)
    noisy = rng.random(n) < 0.1
    y[noisy] = rng.integers(0, C, int(noisy.sum()))
    if name == "c4_absent":
        y[y == 1] = 3
    w, s = bagging_inputs(n, d, T, depth, seed=T + depth)
    return X, y, w, s, C, T, depth


@functools.lru_cache(maxsize=None)
def _reference(name):
    X, y, w, s, C, T, depth = _data(name)
    thr, sf, st, lc = M.train_classifier(X, y, w, s, C, max_depth=depth)
    return thr, sf, M.heap_arrays(sf, st, lc)


def _check_thresholds(F, thr):
    t_dev, ns_dev = (a.cpu().numpy() for a in F.split_thresholds)
    for f, t in enumerate(thr):
        assert ns_dev[f] == t.size
        assert np.array_equal(t_dev[f, :t.size], t.astype(np.float32))


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_train_matches_reference(cuda, name):
    from dal.random_forest import train_classifier

    X, y, w, s, C, T, depth = _data(name)
    thr, sf, (inner, leaf) = _reference(name)
    splits = (sf >= 0).sum(axis=1)
    assert (splits >= (9 if depth >= 4 else 2)).all(), splits  # the trees are real trees
    F = train_classifier(X, y, T, max_depth=depth, weights=w, feature_subsets=s, device=cuda, num_classes=C)
    assert F.n_classes == C and F.depth == depth
    assert np.array_equal(F.inner, inner)
    assert np.array_equal(F.leaf, leaf)
    _check_thresholds(F, thr)
    if name == "c4_absent":
        assert not (F.leaf == 1).any()


@pytest.mark.parametrize("case", ["min_instances", "min_gain", "bins4", "bins100", "depth1", "constant_feature",
                                  "one_class", "heavy_weights"])
def test_gpu_train_edge_cases_match_reference(cuda, case):
    """MLlib's strategy knobs and degenerate inputs on c10's data."""
    from dal.random_forest import bagging_inputs, train_classifier

    X, y, w, s, C, T, depth = _data("c10")
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
        w, s = bagging_inputs(X.shape[0], X.shape[1], T, depth, seed=T + depth)
    elif case == "constant_feature":
        X = X.copy()
        X[:, 0] = 0.5
        X[:, 3] = -2.0
    elif case == "one_class":
        y = np.full(X.shape[0], 7, dtype=np.int64)
    elif case == "heavy_weights":
        w = (w * 37).astype(np.int32)
    F = train_classifier(X, y, T, max_depth=depth, max_bins=max_bins, weights=w, feature_subsets=s, device=cuda,
                         num_classes=C, **kw)
    thr, sf, st, lc = M.train_classifier(X, y, w, s, C, max_depth=depth, max_bins=max_bins, **rkw)
    inner, leaf = M.heap_arrays(sf, st, lc)
    assert np.array_equal(F.inner, inner)
    assert np.array_equal(F.leaf, leaf)
    _check_thresholds(F, thr)
    if case == "one_class":
        assert (sf < 0).all() and (F.leaf == 7).all()  # a root leaf of that class


def _raw_train(cuda, X, y, w, s, depth, n_classes):
    """dal_rf_find_splits + one of the two training entries through the C ABI
    (n_classes None: dal_rf_train): (inner, leaf) bytes."""
    import torch

    from dal import _lib
    from dal.random_forest import num_splits

    lib = _lib.load()
    n, d = X.shape
    T, n_inner, m = w.shape[0], (1 << depth) - 1, s.shape[2]
    ns = num_splits(n)
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(cuda)  # noqa: E731
    x, lab, wt, sub = dev(X, np.float32), dev(y, np.uint8), dev(w, np.int32), dev(s, np.int32)
    thr = torch.empty((d, _lib.DAL_RF_MAX_SPLITS), dtype=torch.float32, device=cuda)
    cnt = torch.empty(d, dtype=torch.int32, device=cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    st = torch.cuda.current_stream(cuda).cuda_stream
    _lib.call("dal_rf_find_splits", x.data_ptr(), n, d, d, 0, n, ns, thr.data_ptr(), cnt.data_ptr(),
              status.data_ptr(), st)
    wsb = int(lib.dal_rf_train_workspace_bytes(n, d, T, depth, m, ns) if n_classes is None else
              lib.dal_rf_train_multiclass_workspace_bytes(n, d, T, depth, m, ns, n_classes))
    assert wsb > 0
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device=cuda)
    wsp = (ws.data_ptr() + 255) // 256 * 256
    inner = torch.full((T, n_inner, 2), -7, dtype=torch.int32, device=cuda)
    leaf = torch.full((T, n_inner + 1), 99, dtype=torch.uint8, device=cuda)
    head = (x.data_ptr(), n, d, d, lab.data_ptr(), thr.data_ptr(), cnt.data_ptr(), ns, wt.data_ptr(),
            sub.data_ptr(), m, T, depth, 1, 0.0)
    tail = (inner.data_ptr(), leaf.data_ptr(), wsp, wsb, st)
    if n_classes is None:
        _lib.call("dal_rf_train", *head, *tail)
    else:
        _lib.call("dal_rf_train_multiclass", *head, n_classes, *tail)
    assert int(status.item()) == 0
    return inner.cpu().numpy().tobytes(), leaf.cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def _two_class_set():
    from dal.random_forest import bagging_inputs

    g = load_golden("checkerboard4x4.npz")
    X, y = g["X"], g["y"].astype(np.int64)
    w, s = bagging_inputs(X.shape[0], X.shape[1], 10, 4, seed=14)
    return X, y, w, s


def test_two_classes_equal_the_binary_oracle(cuda):
    """The binary entry runs the C-class kernels at C = 2, so the yardstick of
    the two-class fit is the binary CPU restatement (oracle/rf_oracle.py), byte
    for byte, not the other entry."""
    from oracle import rf_oracle

    X, y, w, s = _two_class_set()
    _, sf, st, lc = rf_oracle.train_classifier(X, y, w, s, max_depth=4)
    assert ((sf >= 0).sum(axis=1) >= 9).all()  # real trees
    inner = np.zeros(sf.shape + (2,), dtype=np.int32)
    inner[..., 1] = np.array([np.inf], dtype=np.float32).view(np.int32)[0]
    inner[..., 0][sf >= 0] = sf[sf >= 0]
    inner[..., 1][sf >= 0] = st[sf >= 0].astype(np.float32).view(np.int32)
    assert _raw_train(cuda, X, y, w, s, 4, 2) == (inner.tobytes(), lc.astype(np.uint8).tobytes())


def test_two_classes_equal_the_binary_entry(cuda):
    X, y, w, s = _two_class_set()
    assert _raw_train(cuda, X, y, w, s, 4, 2) == _raw_train(cuda, X, y, w, s, 4, None)


def test_repeated_fit_is_identical(cuda):
    X, y, w, s, C, T, depth = _data("c32_deep")
    a = _raw_train(cuda, X, y, w, s, depth, C)
    assert a == _raw_train(cuda, X, y, w, s, depth, C)
    _, _, (inner, leaf) = _reference("c32_deep")
    assert a == (inner.tobytes(), leaf.tobytes())


def test_trained_forest_drives_the_score_kernels(cuda):
    from dal.random_forest import predict, train_classifier

    X, y, w, s, C, T, depth = _data("c10")
    _, sf, (inner, leaf) = _reference("c10")
    F = train_classifier(X, y, T, max_depth=depth, weights=w, feature_subsets=s, device=cuda, num_classes=C)
    Xq = np.random.default_rng(8).random((1500, X.shape[1]), dtype=np.float32)
    cnt = R.counts(Forest(inner=inner, leaf=leaf, depth=depth, n_classes=C), Xq)
    pred, counts = predict(F, Xq, device=cuda)
    assert np.array_equal(counts.cpu().numpy(), cnt)
    assert np.array_equal(pred.cpu().numpy(), R.pred(cnt))
    own, _ = predict(F, X, device=cuda)
    assert (own.cpu().numpy() == y).mean() > 0.5


@functools.lru_cache(maxsize=None)
def _loop_pool(first_window_lacks_a_class):
    rng = np.random.default_rng(17)
    X = rng.random((600, 8)).astype(np.float32)
    y = (X[:, 0] * 3).astype(int).clip(0, 2) * 2 + 5  # labels 5, 7, 9
    if first_window_lacks_a_class:
        order = np.argsort(y == 9, kind="stable")  # every 9 after every 5 and 7
        X, y = X[order], y[order]
        assert set(y[:20].tolist()) == {5, 7}
    else:
        assert set(y[:20].tolist()) == {5, 7, 9}
    return X, y, O.density_canonical(X, np.arange(20))


@pytest.mark.parametrize("lacking", [False, True], ids=["all_classes", "window_lacks_a_class"])
@pytest.mark.parametrize("strategy", ["uncertainty", "information_density"])
def test_run_loop_trains_on_the_gpu(cuda, strategy, lacking):
    """train -> score -> select on the GPU for labels 5, 7, 9: the history and
    the test accuracy equal the same loop with the reference trainer (a
    callable) and the reference selection."""
    from dal.loop import run_loop

    X, y, dens = _loop_pool(lacking)
    seen = []

    def ref_select(strategy_, pool, unlabeled, model, k):
        F = model.forest
        assert F.n_classes == 3
        seen.append(int(F.leaf.max()))
        if strategy_ == "uncertainty":
            return R.select(R.counts(F, pool[unlabeled]), F.n_trees, "least_confidence", unlabeled, k)[0]
        return DW.select(pool, unlabeled, F, k, density=dens)[1]

    kw = dict(X_test=X[300:], y_test=y[300:], strategy=strategy, window_size=20, n_estimators=10,
              max_iterations=3, seed=4)
    got = run_loop(X, y, device=cuda, trainer="gpu", num_classes=3, **kw)
    ref = run_loop(X, y, select_fn=ref_select, trainer=M.loop_trainer(np.unique(y), 3), **kw)
    assert len(got.labeled_history) == 3
    for a, b in zip(got.labeled_history, ref.labeled_history):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert got.accuracy == ref.accuracy  # predict returns labels, not class ids
    if lacking:
        assert seen[0] < 2  # the first forest has three classes but no leaf of the third
