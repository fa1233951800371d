"""C-class forest training without a GPU: the NumPy restatement
(tests/rf_multiclass_reference.py) against the frozen binary oracle and
hand-evaluated cases, the Python checks of dal.random_forest, the argument
checks of dal_rf_train_multiclass (C ABI, before any HIP call) and the loop's
``num_classes`` argument."""
import ctypes

import numpy as np
import pytest

import rf_multiclass_reference as M
from conftest import load_golden
from oracle import rf_oracle as R


def _ones(n):
    return np.ones((1, n), dtype=np.int64)


# ------------------------------------------------- reference vs the oracle --
def _binary_sets():
    g = load_golden("checkerboard4x4.npz")
    yield g["X"][:400], g["y"][:400].astype(np.int64), 10, 4
    rng = np.random.default_rng(3)
    X = rng.random((300, 8)).astype(np.float32)
    yield X, (X[:, 0] + 0.4 * X[:, 5] > 0.7).astype(np.int64), 7, 5


def test_reference_at_two_classes_is_the_oracle():
    from dal.random_forest import bagging_inputs

    for X, y, T, depth in _binary_sets():
        w, s = bagging_inputs(X.shape[0], X.shape[1], T, depth, seed=T + depth)
        thr, sf, st, lc = R.train_classifier(X, y, w, s, max_depth=depth)
        thr2, sf2, st2, lc2 = M.train_classifier(X, y, w, s, 2, max_depth=depth)
        assert (sf >= 0).sum() >= 3 * T
        assert all(np.array_equal(a, b) for a, b in zip(thr, thr2))
        assert np.array_equal(sf, sf2) and np.array_equal(lc, lc2)
        assert np.array_equal(st.view(np.int64), st2.view(np.int64))  # bits, NaN included


# ------------------------------------------------------ hand-evaluated, C = 3 --
def test_separable_three_classes_pure_children():
    # x 0..5, classes 0 0 1 1 2 2, depth 2.  Root counts (2,2,2): imp 2/3.
    # Splits x<=1 and x<=3 both gain 2/3 - (4/6)(1/2) = 1/3; x<=1 comes first.
    # Left child (2,0,0) is pure -> leaf 0; right (0,2,2) splits at x<=3 into pure leaves.
    X = np.arange(6.0)[:, None]
    y = np.array([0, 0, 1, 1, 2, 2])
    _, sf, st, lc = M.train_classifier(X, y, _ones(6), np.zeros((1, 3, 1), dtype=np.int64), 3, max_depth=2)
    assert sf[0].tolist() == [0, -1, 0]
    assert st[0, 0] == 1.0 and np.isnan(st[0, 1]) and st[0, 2] == 3.0
    assert lc[0].tolist() == [0, 0, 1, 2]


def test_equal_features_first_in_subset_order_wins():
    X = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]])
    y = np.array([0, 1, 2])
    for order in ([1, 0], [0, 1]):
        _, sf, _, _ = M.train_classifier(X, y, _ones(3), np.array([[order]]), 3, max_depth=1)
        assert sf[0].tolist() == [order[0]]


def test_labels_independent_of_x_give_a_root_leaf():
    # each x value holds one row of every class: every split leaves the class mix unchanged, gain 0
    X = np.repeat([0.0, 1.0], 3)[:, None]
    y = np.array([0, 1, 2, 0, 1, 2])
    _, sf, _, lc = M.train_classifier(X, y, _ones(6), np.zeros((1, 1, 1), dtype=np.int64), 3, max_depth=1)
    assert sf[0].tolist() == [-1] and lc[0].tolist() == [0, 0]


def test_leaf_tie_goes_to_the_lower_class_id():
    # depth 1: left child x<=0 holds classes (0, 2, 2) by weight -> class 1, not 2;
    # right child holds (3, 0, 0)
    X = np.array([0.0, 0.0, 1.0])[:, None]
    y = np.array([1, 2, 0])
    w = np.array([[2, 2, 3]], dtype=np.int64)
    _, sf, _, lc = M.train_classifier(X, y, w, np.zeros((1, 1, 1), dtype=np.int64), 3, max_depth=1)
    assert sf[0].tolist() == [0] and lc[0].tolist() == [1, 0]
    assert M.predict([0, 2, 2]) == 1 and M.predict([1, 1, 1]) == 0 and M.predict([0, 0, 5]) == 2


def test_gini_class_order_and_empty():
    assert M.gini([0, 0, 0]) == 0.0 and M.gini([4, 0, 0]) == 0.0
    assert M.gini([1, 1, 1]) == ((1.0 - (1 / 3.0) ** 2) - (1 / 3.0) ** 2) - (1 / 3.0) ** 2
    assert M.gini([3, 1]) == R.gini([3, 1])


# ------------------------------------------------------------ Python checks --
def test_check_labels():
    from dal.random_forest import check_labels

    out = check_labels(np.array([0, 2, 1, 2]), 4, 3)
    assert out.dtype == np.uint8 and out.tolist() == [0, 2, 1, 2]
    assert check_labels([0, 1, 1], 3).tolist() == [0, 1, 1]              # the binary default
    assert check_labels(np.arange(32), 32, 32, num_trees=255).size == 32  # the limits themselves
    with pytest.raises(ValueError, match=r"\{0, 1\}"):
        check_labels([0, 2], 2)
    with pytest.raises(ValueError, match="class ids"):
        check_labels([0, 3], 2, 3)
    with pytest.raises(ValueError, match="class ids"):
        check_labels([0, -1], 2, 3)
    with pytest.raises(ValueError, match="class ids"):
        check_labels([0, 1, 2], 4, 3)                                     # wrong length
    for bad in (1, 33):
        with pytest.raises(ValueError, match="num_classes"):
            check_labels([0, 1], 2, bad)
    with pytest.raises(ValueError, match="trees"):
        check_labels([0, 1, 2], 3, 3, num_trees=256)
    check_labels([0, 1], 2, 2, num_trees=1000)                            # binary forests have no tree limit


def test_check_split_histogram_class_factor():
    from dal.random_forest import check_split_histogram

    check_split_histogram(28, 31, 32)           # 28 x 33 x 32 x 4 = 118,272 B: fits
    check_split_histogram(28, 31, n_classes=32)
    with pytest.raises(ValueError, match="split histogram"):
        check_split_histogram(28, 99, 32)       # 28 x 101 x 32 x 4 = 361,984 B
    check_split_histogram(600, 31)              # the binary default is unchanged
    with pytest.raises(ValueError, match="split histogram"):
        check_split_histogram(600, 31, 3)


# --------------------------------------------------------------------- C ABI --
def _train(lib, n=1000, d=784, m=28, T=10, depth=4, ns=31, C=32, null=None, ws_bytes=1 << 40):
    p = [ctypes.c_void_p(256)] * 9  # x labels thresholds n_splits weights subsets out_inner out_leaf ws
    if null is not None:
        p[null] = None
    x, lab, thr, nsp, w, sub, oi, ol, ws = p
    return lib.dal_rf_train_multiclass(x, n, d, d, lab, thr, nsp, ns, w, sub, m, T, depth, 1, 0.0, C, oi, ol, ws,
                                       ws_bytes, None)


def test_abi_rejects_before_any_hip_call():
    from dal import _lib

    lib = _lib.load()
    assert lib.dal_abi_version() == 10
    assert _train(lib, C=33) == -3 and _train(lib, C=1) == -3     # DAL_ERR_UNSUPPORTED
    assert _train(lib, ns=99) == -3                               # 28 x 101 x 32 x 4 B of LDS
    assert _train(lib, m=784, T=1, C=3) == -3                     # one tree: all 784 features
    assert _train(lib, depth=11) == -3
    for i in range(9):
        assert _train(lib, null=i) == -1                          # DAL_ERR_ARG
    assert _train(lib, n=0) == -2 and _train(lib, m=785) == -2 and _train(lib, ns=255) == -2
    # everything valid up to the workspace: 784 features at 32 classes fit the LDS bound
    assert _train(lib, ws_bytes=16) == -2
    ws = lib.dal_rf_train_multiclass_workspace_bytes
    assert ws(1000, 784, 10, 4, 28, 31, 32) > ws(1000, 784, 10, 4, 28, 31, 3) > 0
    assert ws(1000, 784, 10, 4, 28, 31, 2) >= lib.dal_rf_train_workspace_bytes(1000, 784, 10, 4, 28, 31)
    for bad in ((0, 784, 10, 4, 28, 31, 3), (1000, 0, 10, 4, 28, 31, 3), (1000, 784, 0, 4, 28, 31, 3),
                (1000, 784, 10, 0, 28, 31, 3), (1000, 784, 10, 11, 28, 31, 3), (1000, 784, 10, 4, 0, 31, 3),
                (1000, 784, 10, 4, 28, -1, 3), (1000, 784, 10, 4, 28, 31, 1), (1000, 784, 10, 4, 28, 31, 33)):
        assert ws(*bad) == 0


# (n, d, T, depth, m, num_splits): multiclass at C = 2 and 32, regressor at k_y = k_sq = 1 and
# DAL_RF_REG_MAX_LIMBS (8) -- bytes returned by the library of the commit before the trainers'
# shared layout function (rf_layout), which must return the same.  Last column: what
# dal_rf_train_workspace_bytes returned there, before the binary fit ran the C-class kernels
# (their 64 B of scratch per split node came on top).
WORKSPACE_BYTES = [
    ((1, 1, 1, 1, 1, 0), 2048, 2048, 1792, 2304, 1792),                              # n = 1, depth 1
    ((1000, 784, 10, 4, 28, 31), 1424128, 10313728, 1825280, 10122240, 1419008),
    ((5000, 64, 10, 4, 8, 31), 697600, 3251200, 718080, 3101440, 692480),
    ((1025, 64, 2, 6, 8, 31), 215808, 2258688, 422400, 2329088, 211712),
    ((333, 7, 3, 10, 7, 254), 22180352, 352850432, 66267136, 374892544, 22082048),   # DAL_RF_MAX_DEPTH
    ((200000, 64, 10, 4, 8, 31), 20977408, 23531008, 8517888, 10901248, 20972288),
    ((1000, 784, 10, 11, 28, 31), 0, 0, 0, 0, 0),                                    # depth 11: rejected
]


@pytest.mark.parametrize("shape,c2,c32,k1,k8,binary_before", WORKSPACE_BYTES,
                         ids=[str(r[0]) for r in WORKSPACE_BYTES])
def test_workspace_bytes_are_what_they_were(shape, c2, c32, k1, k8, binary_before):
    from dal import _lib

    lib = _lib.load()
    n, d, T, depth, m, ns = shape
    multi, regress = lib.dal_rf_train_multiclass_workspace_bytes, lib.dal_rf_train_regressor_workspace_bytes
    assert multi(*shape, 2) == c2 and multi(*shape, 32) == c32
    assert regress(n, T, depth, m, ns, 1, 1) == k1 and regress(n, T, depth, m, ns, 8, 8) == k8
    assert lib.dal_rf_train_workspace_bytes(*shape) == multi(*shape, 2)
    assert binary_before <= c2


# ----------------------------------------------------------------------- loop --
def test_run_loop_num_classes_argument():
    from dal.loop import run_loop

    rng = np.random.default_rng(0)
    X = rng.random((90, 4)).astype(np.float32)
    y = np.arange(90) % 3
    with pytest.raises(ValueError, match="num_classes=2"):
        run_loop(X, y, strategy="uncertainty", trainer="gpu", num_classes=2, max_iterations=1)
    with pytest.raises(ValueError, match="trainer='gpu'") as e:
        run_loop(X, y, strategy="uncertainty", trainer="gpu", max_iterations=1)
    assert "num_classes=" in str(e.value)
    with pytest.raises(ValueError, match="strategy='density'"):
        run_loop(X, y, strategy="density", trainer="gpu", num_classes=3, max_iterations=1)


def test_loop_trainer_maps_labels_and_predicts_labels():
    """The loop test's reference trainer: labels 5, 7, 9 become ids 0, 1, 2 for
    the fit and come back as labels from predict."""
    rng = np.random.default_rng(5)
    X = rng.random((120, 3)).astype(np.float32)
    y = (X[:, 0] * 3).astype(int).clip(0, 2) * 2 + 5
    model = M.loop_trainer([5, 7, 9], 3)(X, y, 5, 1)
    assert model.forest.n_classes == 3 and set(np.unique(model.forest.leaf).tolist()) <= {0, 1, 2}
    pred = model.predict(X)
    assert set(pred.tolist()) <= {5, 7, 9} and (pred == y).mean() > 0.8
