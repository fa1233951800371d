"""NumPy / Python fp64 restatement of the LAL step's canonical semantics
(dal.active_learner; ActiveLearnerLAL.selectNext of
lal_direct_mllib_implementation/classes/active_learner.py:240-343).

Everything is integers or IEEE fp64 add, multiply and divide in a fixed
order: the two sums (the regressor's tree sum and f6's histogram sum) are
explicit Python loops over Python floats -- never np.sum, which sums pairwise.
The heap arrays of a dal.forest.RegressionForest / Forest are walked as they
stand."""
import math

import numpy as np


def tables(T):
    """(f1, f2) fp64 [T + 1]: active_learner.py:280 and getSD (:232-236)."""
    f1, f2 = [], []
    for v in range(T + 1):
        s = float(v)
        mean = s / T
        f1.append(s / T)
        f2.append(math.sqrt((s * ((1 - mean) ** 2) + (T - s) * (mean ** 2)) / (T - 1)))
    return np.array(f1, dtype=np.float64), np.array(f2, dtype=np.float64)


def regress_leaves(model, X):
    """The leaf every tree gives every row: fp64 [n, TR].  X fp32 or fp64 [n,
    d], compared as fp64: left iff x[feature] <= threshold (NaN goes right)."""
    X = np.asarray(X)
    Xd = X.astype(np.float64)
    n = Xd.shape[0]
    TR, D = model.n_trees, model.depth
    n_inner = (1 << D) - 1
    rows = np.arange(n)
    out = np.empty((n, TR), dtype=np.float64)
    for t in range(TR):
        h = np.zeros(n, dtype=np.int64)
        for _ in range(D):
            f = model.inner_feature[t, h]
            thr = model.inner_threshold[t, h]
            with np.errstate(invalid="ignore"):
                left = Xd[rows, f] <= thr
            h = 2 * h + np.where(left, 1, 2)
        out[:, t] = model.leaf[t, h - n_inner]
    return out


def sum_leaves(leaves, reverse=False):
    """(((0.0 + l_0) + l_1) + ...) / float(TR) per row, a Python float loop
    (``reverse``: the same trees from the last to the first -- the
    discrimination check's wrong order)."""
    n, TR = leaves.shape
    order = range(TR - 1, -1, -1) if reverse else range(TR)
    out = np.empty(n, dtype=np.float64)
    for i in range(n):
        s = 0.0
        row = leaves[i].tolist()
        for t in order:
            s = s + row[t]
        out[i] = s / float(TR)
    return out


def regress(model, X):
    """RandomForestModel.predict of the regression forest: fp64 [n]."""
    return sum_leaves(regress_leaves(model, X))


def votes(forest, X):
    """v_i = the number of trees of the binary dal.forest.Forest voting 1:
    fp32 rows against the heap's fp32 thresholds (x <= t32 <=> x <= t64)."""
    X = np.asarray(X, dtype=np.float32)
    n = X.shape[0]
    D = forest.depth
    n_inner = (1 << D) - 1
    rows = np.arange(n)
    v = np.zeros(n, dtype=np.int64)
    for t in range(forest.n_trees):
        h = np.zeros(n, dtype=np.int64)
        feat = forest.inner[t, :, 0]
        thr = np.ascontiguousarray(forest.inner[t, :, 1]).view(np.float32)
        for _ in range(D):
            with np.errstate(invalid="ignore"):
                left = X[rows, feat[h]] <= thr[h]
            h = 2 * h + np.where(left, 1, 2)
        v += forest.leaf[t, h - n_inner].astype(np.int64)
    return v


def histogram(v, T, mask=None):
    """h[v] = the number of (masked) rows with that vote count: int64 [T + 1]."""
    v = np.asarray(v)
    if mask is not None:
        v = v[np.asarray(mask, dtype=bool)]
    return np.bincount(v, minlength=T + 1).astype(np.int64)


def lal_rows(hist, T, n_labeled, n_positive):
    """The T + 1 feature rows [f1, f2, f3, f6, f8] (active_learner.py:313-314)."""
    f1, f2 = tables(T)
    f3 = float(n_positive) / n_labeled
    s = 0.0
    nU = 0
    for v in range(T + 1):
        s = s + float(int(hist[v])) * float(f2[v])
        nU += int(hist[v])
    f6 = s / float(nU) if nU else float("nan")
    f8 = float(n_labeled)
    rows = np.empty((T + 1, 5), dtype=np.float64)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = f1, f2, f3, f6, f8
    return rows


def order_desc(scores, idx):
    """``idx`` sorted by DESCENDING score, NaN last, -0.0 == +0.0, ties to the
    lower index."""
    s = np.asarray(scores, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    nan = np.isnan(s)
    key = np.where(nan, 0.0, -s) + 0.0  # (-0.0 + 0.0 == +0.0)
    return np.lexsort((idx, key, nan))


def select_lal(X, unlabeled, forest, lal_model, k, n_labeled, n_positive):
    """(scores[U], indices[k], selected_scores[k], votes[U], lut[T + 1])."""
    unl = np.asarray(unlabeled, dtype=np.int64)
    T = forest.n_trees
    v = votes(forest, np.asarray(X)[unl])
    hist = histogram(v, T)
    lut = regress(lal_model, lal_rows(hist, T, n_labeled, n_positive))
    scores = lut[v]
    o = order_desc(scores, unl)[: min(int(k), unl.size)]
    return scores, unl[o], scores[o], v, lut


def bits_equal(a, b):
    """Bit equality of two fp64 (or integer) arrays."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return bool(np.array_equal(a.view(np.int64), b.view(np.int64)))
    return bool(np.array_equal(a, b))
