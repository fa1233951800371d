"""Multiclass uncertainty sampling, host side: the C-class LUTs, the forest
builders' class ids, the unchanged binary defaults, and the new entry point's
argument validation.  CPU only (no kernel launches)."""
import ctypes

import numpy as np
import pytest

import multiclass_reference as R
from conftest import golden_forest, load_golden
from dal import _lib, luts
from dal.forest import Forest
from oracle import dal_oracle as O


@pytest.mark.parametrize("T", [1, 2, 3, 10, 100, 255])
@pytest.mark.parametrize("strategy", luts.STRATEGIES)
def test_multiclass_lut_equals_reference(T, strategy):
    got, ref = luts.multiclass_lut(strategy, T), R.table(strategy, T)
    assert got.dtype == np.float64 and got.shape == (T + 1,)
    assert np.array_equal(got, ref) and np.array_equal(np.signbit(got), np.signbit(ref))
    assert not np.isnan(got).any()
    assert luts.MULTICLASS_ASCENDING[strategy] == R.ASCENDING[strategy]
    if strategy == "entropy":  # h[T] is -0.0; the class-ordered sum from +0.0 is +0.0
        assert got[T] == 0.0 and np.signbit(got[T]) and got[0] == 0.0 and not np.signbit(got[0])


def test_multiclass_lut_rejects_bad_arguments():
    with pytest.raises(ValueError):
        luts.multiclass_lut("entropy", 0)
    with pytest.raises(ValueError):
        luts.multiclass_lut("variance", 10)


def _three_leaf_tree():
    # node 0: x[0] <= 0.5 -> node 1 (leaf, class 2) else node 2: x[1] <= 0.25 -> leaf class 0 else leaf class 1
    feature = [0, -1, 1, -1, -1]
    threshold = [0.5, 0.0, 0.25, 0.0, 0.0]
    left = [1, -1, 3, -1, -1]
    right = [2, -1, 4, -1, -1]
    value = [0, 2, 0, 0, 1]
    return feature, threshold, left, right, value, [0]


def test_from_nodes_n_classes_round_trip():
    F = Forest.from_nodes(*_three_leaf_tree(), n_classes=3)
    assert F.n_classes == 3 and F.depth == 2 and F.leaf.dtype == np.uint8
    assert F.leaf.tolist() == [[2, 2, 0, 1]]  # the shallow leaf pads its subtree with its class
    F.check_classes()
    X = np.array([[0.1, 0.9], [0.9, 0.1], [0.9, 0.9]], dtype=np.float32)
    assert R.counts(F, X).tolist() == [[0, 0, 1], [1, 0, 0], [0, 1, 0]]
    B = Forest.from_nodes(*_three_leaf_tree())  # the binary default: any non-zero value is class 1
    assert B.n_classes == 2 and B.leaf.tolist() == [[1, 1, 0, 1]]
    with pytest.raises(ValueError):
        Forest.from_nodes(*_three_leaf_tree(), n_classes=33)
    f, t, l, r, v, roots = _three_leaf_tree()
    with pytest.raises(ValueError):
        Forest.from_nodes(f, t, l, r, [0, 3, 0, 0, 1], roots, n_classes=3)  # class 3 of 3


def test_check_classes_rejects_a_leaf_outside_the_classes():
    F = Forest.synthetic(5, 3, 8, seed=2, n_classes=6)
    F.check_classes()
    bad = Forest(inner=F.inner, leaf=F.leaf.copy(), depth=F.depth, n_classes=6)
    bad.leaf[3, 2] = 6
    with pytest.raises(ValueError, match="class 6"):
        bad.check_classes()
    with pytest.raises(ValueError):
        Forest(inner=F.inner, leaf=F.leaf, depth=F.depth, n_classes=33).check_classes()


def test_from_sklearn_multiclass_non_contiguous_labels():
    from sklearn.ensemble import RandomForestClassifier

    rng = np.random.default_rng(4)
    X = rng.random((300, 5)).astype(np.float32)
    y = np.array([1, 4, 9])[(X[:, 0] * 3).astype(int).clip(0, 2)]
    rf = RandomForestClassifier(n_estimators=9, max_depth=5, random_state=1).fit(X, y)
    F = Forest.from_sklearn(rf, multiclass=True)
    assert F.n_classes == 3 and F.classes_.tolist() == [1, 4, 9] and F.n_trees == 9
    assert int(F.leaf.max()) <= 2
    hard = np.stack([e.predict(X) for e in rf.estimators_]).astype(int)  # class ids, [T, n]
    ref = np.stack([(hard == c).sum(axis=0) for c in range(3)], axis=1)
    cnt = R.counts(F, X)
    assert np.array_equal(cnt, ref) and (cnt.sum(axis=1) == 9).all()
    # the default stays one-vs-rest on the label
    B = Forest.from_sklearn(rf, positive_label=4)
    assert B.n_classes == 2 and B.classes_ is None
    assert np.array_equal(R.counts(B, X)[:, 1], (hard == 1).sum(axis=0))


MLLIB_TEXT = """TreeEnsembleModel classifier with 2 trees

  Tree 0:
    If (feature 0 <= 0.5)
     Predict: 2.0
    Else (feature 0 > 0.5)
     If (feature 1 <= 0.25)
      Predict: 0.0
     Else (feature 1 > 0.25)
      Predict: 1.0
  Tree 1:
    If (feature 1 <= 0.75)
     Predict: 1.0
    Else (feature 1 > 0.75)
     Predict: 2.0
"""


def test_from_mllib_debug_string_multiclass():
    F = Forest.from_mllib_debug_string(MLLIB_TEXT, n_classes=3)
    assert F.n_classes == 3 and F.n_trees == 2 and F.depth == 2
    assert F.leaf.tolist() == [[2, 2, 0, 1], [1, 1, 2, 2]]
    B = Forest.from_mllib_debug_string(MLLIB_TEXT)  # binary mapping: only ``Predict: 1.0`` is class 1
    assert B.n_classes == 2 and B.leaf.tolist() == [[0, 0, 0, 1], [1, 1, 0, 0]]
    with pytest.raises(ValueError):
        Forest.from_mllib_debug_string(MLLIB_TEXT, n_classes=2)  # ``Predict: 2.0`` is no class of 2


def test_binary_defaults_are_byte_identical():
    """n_classes = 2 and skew = 0 change nothing: the synthetic forest makes
    the draws it always made, and from_nodes keeps the non-zero rule."""
    for seed, dist in ((1, "uniform"), (7, "normal")):
        F = Forest.synthetic(10, 4, 64, seed=seed, dist=dist)
        rng = np.random.default_rng(seed)
        inner = np.zeros((10, 15, 2), dtype=np.int32)
        leaf = np.zeros((10, 16), dtype=np.uint8)
        for t in range(10):
            f = rng.integers(0, 64, size=15)
            th = (rng.random(15) if dist == "uniform" else rng.standard_normal(15)).astype(np.float32)
            inner[t, :, 0], inner[t, :, 1], leaf[t] = f, th.view(np.int32), rng.integers(0, 2, size=16)
        assert F.n_classes == 2 and F.classes_ is None
        assert F.inner.tobytes() == inner.tobytes() and F.leaf.tobytes() == leaf.tobytes()
    g = load_golden("synthetic_512x64_T10.npz")
    of = golden_forest(g)
    args = (of.feature, of.threshold, of.left, of.right, of.value, of.roots)
    a, b = Forest.from_nodes(*args), Forest.from_nodes(*args, n_classes=2)
    assert a.inner.tobytes() == b.inner.tobytes() and a.leaf.tobytes() == b.leaf.tobytes()
    assert set(np.unique(a.leaf)) <= {0, 1}
    assert np.array_equal(R.counts(a, g["X"])[:, 1], O.votes(of, g["X"]))


def test_synthetic_multiclass_and_skew():
    F = Forest.synthetic(50, 4, 16, seed=3, n_classes=7)
    assert F.n_classes == 7 and set(np.unique(F.leaf)) == set(range(7))
    S = Forest.synthetic(255, 4, 16, seed=3, n_classes=32, skew=0.97)
    assert S.n_classes == 32 and (S.leaf == 0).mean() > 0.95 and int(S.leaf.max()) > 0
    S.check_classes()


def test_abi_validation_without_gpu():
    lib = _lib.load()
    assert lib.dal_abi_version() == 10
    assert lib.dal_forest_multiclass_max_classes() == 32 == _lib.DAL_MC_MAX_CLASSES
    p = ctypes.c_void_p(256)

    def score(x=p, n=10, d=4, ldx=4, inner=p, leaf=p, T=10, depth=4, C=3, lut=p, kind=0, flags=None, order=0,
              counts=p, pred=p, scores=p, keys=p):
        return lib.dal_forest_score_multiclass(x, n, d, ldx, inner, leaf, T, depth, C, lut, kind, flags, order,
                                               counts, pred, scores, keys, None)

    for name in ("x", "inner", "leaf", "lut", "scores", "keys"):
        assert score(**{name: None}) == -1, name
    assert score(kind=3) == -1 and score(kind=-1) == -1 and score(order=2) == -1
    assert score(n=-1) == -2 and score(d=0) == -2 and score(ldx=3) == -2
    assert score(C=1) == -3 and score(C=33) == -3
    assert score(T=256) == -3 and score(T=0) == -3
    assert score(depth=17) == -3 and score(depth=0) == -3
    assert score(n=0) == 0                                  # nothing to score: no launch
    assert score(n=0, counts=None, pred=None) == 0          # both optional
    assert score(n=0, C=2, T=255, depth=16) == 0 and score(n=0, C=32, T=1, depth=1) == 0  # the limits themselves


def test_density_weighting_rejects_a_multiclass_forest():
    from dal import density_weighting as dw

    F = Forest.synthetic(10, 4, 8, seed=1, n_classes=3)
    X = np.random.default_rng(0).random((64, 8)).astype(np.float32)
    with pytest.raises(ValueError, match="binary only"):
        dw.select(X, np.arange(10, 64), F, 5)


def test_run_loop_rejects_binary_only_paths_for_multiclass_labels():
    from dal.loop import run_loop

    rng = np.random.default_rng(0)
    X = rng.random((90, 4)).astype(np.float32)
    y = np.arange(90) % 3
    with pytest.raises(ValueError, match="trainer='gpu'"):
        run_loop(X, y, strategy="uncertainty", trainer="gpu", max_iterations=1)
    with pytest.raises(ValueError, match="strategy='density'"):
        run_loop(X, y, strategy="density", trainer="sklearn", max_iterations=1)
