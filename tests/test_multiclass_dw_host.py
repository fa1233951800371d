"""Multiclass information density, host side: the reference's own
definitions, the new entry point's argument validation, and the Python
layers' checks that need no device.  CPU only (no kernel launches)."""
import ctypes

import numpy as np
import pytest

import multiclass_dw_reference as DW
import multiclass_reference as R
from dal import _lib
from dal.forest import Forest
from oracle import dal_oracle as O


def test_reference_two_classes_is_the_two_term_entropy():
    T = 10
    h = R.table("entropy", T)
    cnt = np.array([[T - v, v] for v in range(T + 1)])
    H = DW.entropy(cnt, T)
    for v in range(T + 1):
        assert H[v] == (0.0 + h[T - v]) + h[v]
    assert not np.isnan(H).any() and (H >= 0.0).all() and not np.signbit(H).any()
    assert H[0] == 0.0 and H[T] == 0.0  # a unanimous forest
    one_sided = O.lut_entropy(T)
    assert H[3] != one_sided[3]  # the reference script's score is another function
    d = np.array([2.0, np.nan, -1.5])
    sc = DW.scores(np.array([H[3], H[3], H[5]]), d)
    assert sc[0] == H[3] * 2.0 and np.isnan(sc[1]) and sc[2] == H[5] * -1.5
    assert DW.scores(np.array([H[5]]), np.array([4.0]), beta=0.5)[0] == H[5] * 2.0


def test_reference_selection_order():
    """Descending, NaN last, -0.0 == +0.0 (the lower index first), negatives after zero."""
    sc = np.array([np.nan, 0.0, 0.5, -0.0, -1.0, 0.5, 0.25])
    index = np.array([3, 12, 5, 9, 4, 2, 8])
    idx, sel = DW.select_scores(sc, index, 7)
    assert idx.tolist() == [2, 5, 8, 9, 12, 4, 3]
    assert sel[:3].tolist() == [0.5, 0.5, 0.25] and sel[5] == -1.0 and np.isnan(sel[6])
    idx, _ = DW.select_scores(sc, index, 4)
    assert idx.tolist() == [2, 5, 8, 9]
    keys = DW.score_key(sc)
    assert keys[1] == keys[3] and keys[0] == DW.KEY_NAN
    order = np.lexsort((index, keys))
    assert index[order].tolist() == [2, 5, 8, 9, 12, 4, 3]  # the key order is the reference order


def test_reference_select_uses_counts_density_and_index():
    X = O.synthetic_pool(200, 6, seed=1)
    F = Forest.synthetic(10, 3, 6, seed=5, n_classes=3)
    unl = np.arange(10, 200)
    sc, idx, sel, cnt = DW.select(X, unl, F, 7, excluded=np.arange(10))
    d = O.density_canonical(X, np.arange(10))
    assert np.isnan(d[:10]).all() and not np.isnan(d[10:]).any()
    assert np.array_equal(cnt, R.counts(F, X)[unl]) and np.array_equal(sc, DW.entropy(cnt, 10) * d[unl])
    ref_idx, ref_sel = O.select_topk(sc, unl, 7, ascending=False)
    assert np.array_equal(idx, ref_idx) and np.array_equal(sel, ref_sel)


def test_abi_validation_without_gpu():
    lib = _lib.load()
    assert lib.dal_abi_version() == 10  # a new symbol only
    p = ctypes.c_void_p(256)

    def score(x=p, n=10, d=4, ldx=4, inner=p, leaf=p, T=10, depth=4, C=3, lut=p, density=p, kind=1, derr=0.0,
              flags=None, beta=1.0, counts=p, pred=p, entropy=p, row_index=p, scores=p, keys=p, keys_hi=p):
        return lib.dal_forest_score_multiclass_dw(x, n, d, ldx, inner, leaf, T, depth, C, lut, density, kind, derr,
                                                  flags, beta, counts, pred, entropy, row_index, scores, keys,
                                                  keys_hi, None)

    for name in ("x", "inner", "leaf", "lut", "density", "entropy", "row_index", "scores", "keys"):
        assert score(**{name: None}) == -1, name
    assert score(kind=0) == -1 and score(kind=3) == -1 and score(kind=-1) == -1
    assert score(n=-1) == -2 and score(d=0) == -2 and score(ldx=3) == -2
    assert score(n=1 << 31) == -2                            # row_index is int32
    assert score(C=1) == -3 and score(C=33) == -3
    assert score(T=256) == -3 and score(T=0) == -3
    assert score(depth=17) == -3 and score(depth=0) == -3
    assert score(n=0) == 0                                   # nothing to score: no launch
    assert score(n=0, kind=2) == 0                           # DAL_DENSITY_EXACT
    assert score(n=0, counts=None, pred=None, keys_hi=None) == 0  # the optional outputs
    assert score(n=0, C=2, T=255, depth=16) == 0 and score(n=0, C=32, T=1, depth=1) == 0  # the limits themselves


def test_select_multiclass_checks_the_forest_before_any_device_work():
    from dal import density_weighting as dw

    X = np.random.default_rng(0).random((64, 8)).astype(np.float32)
    unl = np.arange(10, 64)
    F = Forest.synthetic(10, 4, 8, seed=1, n_classes=3)
    bad = Forest(inner=F.inner, leaf=F.leaf.copy(), depth=F.depth, n_classes=3)
    bad.leaf[2, 5] = 3
    with pytest.raises(ValueError, match="class 3"):
        dw.select_multiclass(X, unl, bad, 5)
    big = Forest.synthetic(256, 2, 8, seed=1, n_classes=3)
    with pytest.raises(ValueError, match="at most 255 trees"):
        dw.select_multiclass(X, unl, big, 5)
    assert "select_multiclass" in dw.__all__


def test_sharded_selection_knows_the_new_density_mode():
    """mode="dw" stays binary; "dw_multiclass" is a density mode of its own
    (normalises, keeps the zero-norm check)."""
    from dal import parallel

    assert parallel.DENSITY_MODES == ("dw", "dw_multiclass")


def test_run_loop_information_density_on_the_cpu():
    """run_loop(strategy="information_density") with the reference as
    select_fn: three classes, scikit-learn trainer, no device."""
    from dal.loop import run_loop

    rng = np.random.default_rng(17)
    X = rng.random((300, 8)).astype(np.float32)
    y = (X[:, 0] * 3).astype(int).clip(0, 2) * 2 + 5
    assert len(set(y[:20].tolist())) == 3
    E = np.arange(20)
    dens = O.density_canonical(X, E)
    seen = []

    def ref_select(strategy, pool, unlabeled, model, k):
        assert strategy == "information_density"
        F = Forest.from_sklearn(model, multiclass=True)
        assert F.n_classes == 3
        seen.append(k)
        return DW.select(pool, unlabeled, F, k, density=dens)[1]

    res = run_loop(X, y, strategy="information_density", window_size=20, n_estimators=10, max_iterations=3, seed=4,
                   trainer="sklearn", select_fn=ref_select)
    assert seen == [20, 20, 20] and len(res.labeled_history) == 3
    chosen = np.concatenate(res.labeled_history)
    assert np.unique(chosen).size == 60 and chosen.min() >= 20
