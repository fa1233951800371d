"""LAL query selection, host side: the fp64 tables, the RegressionForest
builders, the new C entry points' argument checks (no device is touched) and
the loop's strategy plumbing."""
import ctypes
import types

import numpy as np
import pytest

import lal_reference as L
from conftest import load_golden
from dal import _lib, loop
from dal.forest import RegressionForest

NEW_SYMBOLS = ("dal_forest_regress_chunk_trees", "dal_forest_regress", "dal_vote_histogram", "dal_lal_rows",
               "dal_votes_rescore")


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize("T", [2, 3, 10, 50, 100])
def test_lal_tables(T):
    from dal.active_learner import lal_tables

    f1, f2 = lal_tables(T)
    r1, r2 = L.tables(T)
    assert f1.dtype == np.float64 and f2.dtype == np.float64 and f1.shape == (T + 1,)
    assert L.bits_equal(f1, r1) and L.bits_equal(f2, r2)
    assert f2[0] == 0.0 and f2[T] == 0.0


def test_lal_tables_one_tree_raises():
    from dal.active_learner import lal_tables

    with pytest.raises(ValueError):
        lal_tables(1)


# ---------------------------------------------------------------- builders
def test_from_nodes_pads_shallow_leaf():
    # tree 0: root splits on feature 1 at 0.3; left child is a leaf (2.5), the
    # right child splits on feature 0 at 0.1 + 2^-60-ish (not fp32) into leaves
    thr = 0.1 + 1e-17
    F = RegressionForest.from_nodes(feature=[1, -1, 0, -1, -1], threshold=[0.3, 0.0, thr, 0.0, 0.0],
                                    left=[1, -1, 3, -1, -1], right=[2, -1, 4, -1, -1],
                                    value=[0.0, 2.5, 0.0, -1.0, 7.0], roots=[0])
    assert F.depth == 2 and F.n_trees == 1
    assert F.inner_feature.dtype == np.int32 and F.inner_feature.shape == (1, 3)
    assert F.inner_threshold.dtype == np.float64 and F.leaf.dtype == np.float64 and F.leaf.shape == (1, 4)
    assert F.inner_feature[0].tolist() == [1, 0, 0]
    assert F.inner_threshold[0, 0] == 0.3 and F.inner_threshold[0, 2] == thr  # not rounded
    assert np.isposinf(F.inner_threshold[0, 1])  # the shallow leaf's padded split: always left
    assert F.leaf[0].tolist() == [2.5, 2.5, -1.0, 7.0]


def _chain(depth):
    """One tree that is a right-going chain of ``depth`` splits."""
    feat, thr, lft, rgt, val = [], [], [], [], []
    for lv in range(depth):
        feat += [0, -1]
        thr += [float(lv), 0.0]
        lft += [2 * lv + 1, -1]
        rgt += [2 * lv + 2, -1]
        val += [0.0, float(lv)]
    feat.append(-1), thr.append(0.0), lft.append(-1), rgt.append(-1), val.append(99.0)
    return feat, thr, lft, rgt, val, [0]


def test_depth_limit():
    assert RegressionForest.from_nodes(*_chain(10)).depth == 10
    with pytest.raises(ValueError):
        RegressionForest.from_nodes(*_chain(11))
    with pytest.raises(ValueError):
        RegressionForest.synthetic(2, 11, 5)


@pytest.mark.parametrize("max_depth", [3, 5])
def test_from_sklearn_leaf_for_leaf(max_depth):
    from sklearn.ensemble import RandomForestRegressor

    rng = np.random.default_rng(max_depth)
    X = rng.random((300, 6)).astype(np.float32)
    y = np.sin(6 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.1 * rng.standard_normal(300)
    rf = RandomForestRegressor(n_estimators=7, max_depth=max_depth, random_state=0).fit(X, y)
    F = RegressionForest.from_sklearn(rf)
    assert F.depth == max_depth and F.n_trees == 7
    Xq = rng.random((200, 6)).astype(np.float32)
    leaves = L.regress_leaves(F, Xq)
    for t, est in enumerate(rf.estimators_):
        assert L.bits_equal(leaves[:, t], est.predict(Xq).astype(np.float64))


DEBUG_STRING = """TreeEnsembleModel regressor with 2 trees

  Tree 0:
    If (feature 0 <= 0.5)
     If (feature 3 <= 0.30000000000000004)
      Predict: -0.0125
     Else (feature 3 > 0.30000000000000004)
      Predict: 0.25
    Else (feature 0 > 0.5)
     Predict: 1.0E-4
  Tree 1:
    Predict: 3.5
"""


def test_from_mllib_debug_string():
    F = RegressionForest.from_mllib_debug_string(DEBUG_STRING)
    assert F.n_trees == 2 and F.depth == 2
    assert F.inner_feature[0].tolist() == [0, 3, 0]
    assert F.inner_threshold[0, 1] == 0.30000000000000004 and np.isposinf(F.inner_threshold[0, 2])
    assert F.leaf[0].tolist() == [-0.0125, 0.25, 1.0e-4, 1.0e-4]
    assert F.leaf[1].tolist() == [3.5] * 4 and np.isposinf(F.inner_threshold[1]).all()
    X = np.array([[0.5, 0, 0, 0.30000000000000004, 0], [0.5, 0, 0, 0.3000000000000001, 0], [0.6, 0, 0, 0, 0]])
    assert L.regress_leaves(F, X)[:, 0].tolist() == [-0.0125, 0.25, 1.0e-4]
    with pytest.raises(ValueError):
        RegressionForest.from_mllib_debug_string(
            "  Tree 0:\n    If (feature 0 in {1.0})\n     Predict: 0.5\n    Else (feature 0 not in {1.0})\n"
            "     Predict: 1.5\n")


def test_from_mllib_saved_round_trip(tmp_path):
    from test_forest_format import write_mllib_saved

    src = RegressionForest.synthetic(5, 3, 5, seed=4)
    n_inner = 7
    feat, thr, lft, rgt, val, roots = [], [], [], [], [], []
    for t in range(src.n_trees):  # the complete heap as node arrays
        base = len(feat)
        roots.append(base)
        for h in range(n_inner):
            feat.append(int(src.inner_feature[t, h])), thr.append(float(src.inner_threshold[t, h]))
            lft.append(base + 2 * h + 1), rgt.append(base + 2 * h + 2), val.append(0.0)
        for leaf in src.leaf[t]:
            feat.append(-1), thr.append(0.0), lft.append(-1), rgt.append(-1), val.append(float(leaf))
    of = types.SimpleNamespace(feature=np.array(feat), threshold=np.array(thr), left=np.array(lft),
                               right=np.array(rgt), value=np.array(val), roots=np.array(roots))
    write_mllib_saved(of, str(tmp_path))
    F = RegressionForest.from_mllib_saved(str(tmp_path))
    assert F.depth == src.depth
    assert np.array_equal(F.inner_feature, src.inner_feature)
    assert L.bits_equal(F.inner_threshold, src.inner_threshold) and L.bits_equal(F.leaf, src.leaf)


def test_check_features():
    F = RegressionForest.synthetic(3, 4, 5, seed=1)
    F.check_features(5)
    with pytest.raises(ValueError, match="outside"):
        F.check_features(int(F.inner_feature.max()))


# --------------------------------------------------------------- C entries
def test_abi_and_symbols():
    lib = _lib.load()
    assert lib.dal_abi_version() == 10
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def test_chunk_trees():
    lib = _lib.load()
    c = [lib.dal_forest_regress_chunk_trees(d) for d in range(1, 11)]
    assert all(v >= 1 for v in c)
    assert all(a >= b for a, b in zip(c, c[1:]))


def test_entry_points_reject_bad_arguments():
    """Negative statuses before any launch: the pointers here are host
    buffers and no device is needed."""
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    ok = dict(x=p, dt=_lib.DAL_X_F64, n=4, d=5, ldx=5, f=p, t=p, leaf=p, nt=3, depth=2, out=p)

    def regress(**kw):
        a = dict(ok, **kw)
        return lib.dal_forest_regress(a["x"], a["dt"], a["n"], a["d"], a["ldx"], a["f"], a["t"], a["leaf"], a["nt"],
                                      a["depth"], a["out"], None)

    for bad in (dict(x=None), dict(f=None), dict(t=None), dict(leaf=None), dict(out=None), dict(depth=0),
                dict(depth=11), dict(nt=0), dict(dt=2)):
        assert regress(**bad) < 0, bad
    assert regress(n=0) == 0  # nothing to do, nothing launched
    assert lib.dal_vote_histogram(None, None, 4, 10, p, None) < 0
    assert lib.dal_vote_histogram(p, None, 4, 10, None, None) < 0
    assert lib.dal_vote_histogram(p, None, 4, 0, p, None) < 0
    assert lib.dal_vote_histogram(p, None, 0, 10, p, None) == 0
    for bad in ((None, p, p, 10, p), (p, None, p, 10, p), (p, p, None, 10, p), (p, p, p, 10, None), (p, p, p, 0, p)):
        h, f1, f2, T, rows = bad
        assert lib.dal_lal_rows(h, f1, f2, T, 0.5, 10.0, rows, None) < 0, bad
    for bad in ((None, p, 10, p, p), (p, None, 10, p, p), (p, p, 10, None, p), (p, p, 10, p, None), (p, p, 0, p, p)):
        v, lut, T, sc, keys = bad
        assert lib.dal_votes_rescore(v, None, 4, lut, T, _lib.DAL_DESCENDING, sc, keys, None) < 0, bad
    assert lib.dal_votes_rescore(p, None, 4, p, 10, 2, p, p, None) < 0
    assert lib.dal_votes_rescore(p, None, 0, p, 10, _lib.DAL_DESCENDING, p, p, None) == 0


# --------------------------------------------------------------------- loop
def test_loop_lal_argument_errors():
    g = load_golden("checkerboard2x2.npz")
    X, y = g["X"], g["y"]
    with pytest.raises(ValueError, match="lal_model"):
        loop.run_loop(X, y, strategy="lal", trainer="sklearn", max_iterations=1)
    y3 = y.copy()
    y3[::3] = 2
    with pytest.raises(ValueError, match="binary"):
        loop.run_loop(X, y3, strategy="lal", trainer="sklearn", max_iterations=1,
                      lal_model=RegressionForest.synthetic(3, 2, 5))
    with pytest.raises(ValueError, match="binary"):
        loop.run_loop(X, y, strategy="lal", trainer="gpu", num_classes=3, max_iterations=1,
                      lal_model=RegressionForest.synthetic(3, 2, 5))


def test_loop_hands_lal_to_select_fn():
    g = load_golden("checkerboard2x2.npz")
    X, y = g["X"], g["y"]
    seen = []

    def select_fn(strategy, pool, unlabeled, model, k):
        seen.append(strategy)
        return unlabeled[:k]

    res = loop.run_loop(X, y, X, y, strategy="lal", window_size=10, max_iterations=3, select_fn=select_fn,
                        trainer="sklearn", lal_model=RegressionForest.synthetic(3, 2, 5))
    assert seen == ["lal"] * 3
    n = X.shape[0]
    assert res.log[0] == f"labeled =  10  unlabeled =  {n - 10}"
    assert res.log[1].startswith("Iteration  1  -- accu =  ")
    assert res.log[2] == f"labeled =  20  unlabeled =  {n - 20}"
    assert len(res.labeled_history) == 3


# ------------------------------------------------------- discrimination
@pytest.mark.parametrize("TR", [7, 200])
def test_reordered_sum_differs_in_bits(TR):
    """The GPU parity test can see a reordered tree sum only if, for its leaf
    values (+-10^e, e in -8..3), another order gives other bits: the reverse
    order must differ from the canonical one on at least a quarter of 1,000
    rows."""
    F = RegressionForest.synthetic(TR, 4, 5, seed=11)
    X = np.random.default_rng(3).random((1000, 5))
    leaves = L.regress_leaves(F, X)
    fwd, rev = L.sum_leaves(leaves), L.sum_leaves(leaves, reverse=True)
    differ = np.count_nonzero(fwd.view(np.int64) != rev.view(np.int64))
    assert differ >= 250, differ
