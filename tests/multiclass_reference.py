"""Test-side restatement of the canonical multiclass uncertainty scores (the
oracle module is frozen and binary; this adds the C-class definitions).

A forest has T trees (1 <= T <= 255) whose leaves are classes c in {0..C-1}
(2 <= C <= 32); a row goes left at a node when x[f] <= thr, thr the fp32
threshold of the device layout (dal.forest rounds fp64 thresholds toward
-inf, so the fp32 compare is the fp64 one for fp32 rows).

  n_c(i)   trees whose leaf for row i is class c          sum_c n_c = T
  pred(i)  the smallest c with maximal n_c

One table of T + 1 Python floats per strategy:

  least_confidence  lc[v] = v / T                    score = lc[max_c n_c]      ascending
  margin            mg[m] = m / T                    score = mg[n_(1) - n_(2)]  ascending
  entropy           h[0] = 0.0,                      score = s after
                    h[v] = -(v/T) * (log(v/T)/log(2))  s = 0.0; s = s + h[n_c], c = 0..C-1
                                                                               descending

Selection: oracle.select_topk (score in order, -0.0 == +0.0, ties to the
lower global index, take k).
"""
import math

import numpy as np

from oracle import dal_oracle as O

ASCENDING = {"least_confidence": True, "margin": True, "entropy": False}
STRATEGIES = tuple(ASCENDING)


def tree_leaves(inner, leaf, depth, X):
    """Class of every tree's leaf for every row: [T, n] from the heap arrays
    inner [T, 2^depth - 1, 2] (feature, fp32 threshold bits), leaf [T, 2^depth]."""
    X = np.asarray(X, dtype=np.float32)
    n, rows = X.shape[0], np.arange(X.shape[0])
    feat = inner[:, :, 0]
    thr = np.ascontiguousarray(inner[:, :, 1]).view(np.float32)
    n_inner = (1 << depth) - 1
    out = np.empty((inner.shape[0], n), dtype=np.int64)
    for t in range(inner.shape[0]):
        h = np.zeros(n, dtype=np.int64)
        for _ in range(depth):
            left = X[rows, feat[t, h]] <= thr[t, h]
            h = 2 * h + np.where(left, 1, 2)
        out[t] = leaf[t, h - n_inner]
    return out


def counts(forest, X):
    """n_c(i) as int64 [n, C]; a leaf class >= C is counted for no class."""
    lv = tree_leaves(forest.inner, forest.leaf, forest.depth, X)
    C = int(forest.n_classes)
    out = np.zeros((lv.shape[1], C), dtype=np.int64)
    for c in range(C):
        out[:, c] = (lv == c).sum(axis=0)
    return out


def table(strategy, T):
    if strategy in ("least_confidence", "margin"):
        return np.array([v / T for v in range(T + 1)], dtype=np.float64)
    if strategy == "entropy":
        return np.array([0.0] + [-(v / T) * (math.log(v / T) / math.log(2)) for v in range(1, T + 1)],
                        dtype=np.float64)
    raise ValueError(strategy)


def pred(cnt):
    return np.argmax(cnt, axis=1)  # (the first maximum: the lowest class)


def scores(cnt, T, strategy):
    tab = table(strategy, T)
    if strategy == "least_confidence":
        return tab[cnt.max(axis=1)]
    if strategy == "margin":
        top = np.sort(cnt, axis=1)
        return tab[top[:, -1] - top[:, -2]]
    s = np.zeros(cnt.shape[0], dtype=np.float64)
    for c in range(cnt.shape[1]):
        s = s + tab[cnt[:, c]]
    return s


def select(cnt, T, strategy, index, k):
    """(indices, their scores) of the k best rows; cnt and index row-aligned."""
    sc = scores(cnt, T, strategy)
    return O.select_topk(sc, np.asarray(index, dtype=np.int64), k, ASCENDING[strategy])
