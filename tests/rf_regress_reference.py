"""Test-side restatement of MLlib 2.1's RandomForest.trainRegressor
(impurity "variance", continuous features) with the project's canonical
statistics, on Python integers.

Thresholds, bins and the invalid-gain marker are the oracle's
(oracle.rf_oracle: num_splits, find_splits, bin_values, INVALID_GAIN); growth,
the first-maximum rule and the leaf rules are those of the classifier
restatements (tests/rf_multiclass_reference.py).  What is new:

  statistics  of a row set R: count = sum w (integer); sum = RN(sum w y);
              sumSq = RN(sum w fl(y y)).  The sums are exact: every label (and
              every fl(y y)) is a dyadic rational, held here as a Python
              integer in units of a common power of two, so sums are integer
              sums, and ``float(int)`` scaled by ``math.ldexp`` is the single
              rounding to nearest-even fp64.  Left statistics of split k: the
              rows with bin <= k; right: exact node sums minus exact left sums,
              rounded once.
  impurity    Variance.calculate: 0 when count == 0, else
              (sumSq - (sum * sum) / count) / count, Python floats in that order
  gain        impurity - (lc/tc) * imp_l - (rc/tc) * imp_r; invalid when a
              child's count < minInstancesPerNode or gain < minInfoGain
  leaf        sum / count (0 when count == 0)
  "auto"      all features for one tree, ceil(d / 3) for a forest

The bagging weights and per-node feature subsets are inputs, so the GPU trainer
is compared on identical draws, byte for byte."""
import math
from fractions import Fraction

import numpy as np

from oracle.rf_oracle import INVALID_GAIN, bin_values, find_splits, num_splits


class Dyadic:
    """A vector of finite doubles as Python integers in units of 2^-shift."""

    def __init__(self, values):
        fr = [Fraction(float(v)) for v in values]
        self.shift = max([f.denominator.bit_length() - 1 for f in fr], default=0)
        self.ints = [int(f * (1 << self.shift)) for f in fr]

    def to_float(self, total: int) -> float:
        """RN(total * 2^-shift): float(int) rounds to nearest even once; the
        scaling by a power of two is exact (no test reaches the subnormals)."""
        return math.ldexp(float(total), -self.shift)


def exact_sum(values, weights) -> float:
    """RN(sum_i weights[i] * values[i]) with the sum exact."""
    d = Dyadic(values)
    return d.to_float(sum(int(w) * v for w, v in zip(weights, d.ints)))


def squares(y):
    """fl(y * y) per label (one IEEE multiply each)."""
    return [float(v) * float(v) for v in y]


def variance(count: int, s: float, sq: float) -> float:
    if count == 0:
        return 0.0
    c = float(count)
    return (sq - (s * s) / c) / c


def subset_size(n_features: int, n_trees: int) -> int:
    """featureSubsetStrategy "auto" for regression: all for one tree, onethird for a forest."""
    return n_features if n_trees == 1 else int(math.ceil(n_features / 3.0))


def train_tree(bins, dy, dq, weights, subsets, n_splits_f, max_depth, min_instances=1, min_info_gain=0.0):
    """One tree.  bins [n, d]; dy, dq: Dyadic labels and squared labels;
    weights int [n]; subsets [2^maxDepth - 1, m].  Returns (split_feature
    [n_inner] (-1 = none), split_bin [n_inner], leaf_value fp64 [n_leaf])
    with a shallow leaf's value filling its subtree."""
    n_inner = (1 << max_depth) - 1
    split_feature = np.full(n_inner, -1, dtype=np.int64)
    split_bin = np.zeros(n_inner, dtype=np.int64)
    leaf_value = np.zeros(1 << max_depth, dtype=np.float64)
    w_all = [int(v) for v in weights]
    node = [0] * len(w_all)
    bins_l = np.asarray(bins).tolist()
    level_nodes = {0: False}  # heap index -> preset leaf flag
    for level in range(max_depth + 1):
        nxt = {}
        for h, preset_leaf in sorted(level_nodes.items()):
            rows = [i for i, w in enumerate(w_all) if w > 0 and node[i] == h]
            tc = sum(w_all[i] for i in rows)
            ts = sum(w_all[i] * dy.ints[i] for i in rows)
            tq = sum(w_all[i] * dq.ints[i] for i in rows)
            best_gain, best = INVALID_GAIN, None
            if not preset_leaf and level < max_depth:
                parent_imp = variance(tc, dy.to_float(ts), dq.to_float(tq))
                for f in subsets[h]:
                    f = int(f)
                    ns = int(n_splits_f[f])
                    hc, hs, hq = [0] * (ns + 1), [0] * (ns + 1), [0] * (ns + 1)
                    for i in rows:
                        b = bins_l[i][f]
                        hc[b] += w_all[i]
                        hs[b] += w_all[i] * dy.ints[i]
                        hq[b] += w_all[i] * dq.ints[i]
                    lc = ls = lq = 0
                    for k in range(ns):
                        lc += hc[k]
                        ls += hs[k]
                        lq += hq[k]
                        rc = tc - lc
                        if lc < min_instances or rc < min_instances:
                            continue
                        li = variance(lc, dy.to_float(ls), dq.to_float(lq))
                        ri = variance(rc, dy.to_float(ts - ls), dq.to_float(tq - lq))
                        lw = lc / float(tc)
                        rw = rc / float(tc)
                        gain = parent_imp - lw * li - rw * ri
                        if gain < min_info_gain:
                            continue
                        if gain > best_gain:
                            best_gain, best = gain, (f, k, li, ri)
            if preset_leaf or level == max_depth or best_gain <= 0:
                span = 1 << (max_depth - level)
                first = (h + 1) * span - 1 - n_inner
                leaf_value[first:first + span] = dy.to_float(ts) / float(tc) if tc else 0.0
                continue
            f, k, li, ri = best
            split_feature[h] = f
            split_bin[h] = k
            child_leaf = level + 1 == max_depth
            nxt[2 * h + 1] = child_leaf or li == 0.0
            nxt[2 * h + 2] = child_leaf or ri == 0.0
            for i in rows:
                node[i] = 2 * h + 1 + (1 if bins_l[i][f] > k else 0)
        level_nodes = nxt
        if not level_nodes:
            break
    return split_feature, split_bin, leaf_value


def train_regressor(X, y, weights, subsets, max_depth=4, max_bins=32, min_instances=1, min_info_gain=0.0):
    """trainRegressor on given bagging weights [T, n] and feature subsets
    [T, 2^maxDepth - 1, m]: (thresholds per feature (list of fp64 arrays),
    split_feature int64 [T, n_inner] (-1 = none), heap arrays (inner_feature
    int32, inner_threshold fp64, leaf fp64) in dal.forest.RegressionForest's
    padded layout).  X fp32 or fp64, used as fp64 without rounding."""
    X = np.asarray(X, dtype=np.float64)
    y = [float(v) for v in np.asarray(y, dtype=np.float64)]
    n, d = X.shape
    ns = num_splits(n, max_bins)
    thresholds = [find_splits(X[:, f], ns) for f in range(d)]
    n_splits_f = np.array([t.size for t in thresholds], dtype=np.int64)
    bins = np.stack([bin_values(X[:, f], thresholds[f]) for f in range(d)], axis=1)
    dy, dq = Dyadic(y), Dyadic(squares(y))
    T = weights.shape[0]
    n_inner = (1 << max_depth) - 1
    sf = np.full((T, n_inner), -1, dtype=np.int64)
    inner_feature = np.zeros((T, n_inner), dtype=np.int32)
    inner_threshold = np.full((T, n_inner), np.inf, dtype=np.float64)
    leaf = np.zeros((T, 1 << max_depth), dtype=np.float64)
    for t in range(T):
        f_, b_, l_ = train_tree(bins, dy, dq, weights[t], subsets[t], n_splits_f, max_depth, min_instances,
                                min_info_gain)
        sf[t], leaf[t] = f_, l_
        for h in np.nonzero(f_ >= 0)[0]:
            inner_feature[t, h] = f_[h]
            inner_threshold[t, h] = thresholds[f_[h]][b_[h]]
    return thresholds, sf, (inner_feature, inner_threshold, leaf)


def heap_forest(arrays):
    """The heap arrays as a dal.forest.RegressionForest."""
    from dal.forest import RegressionForest

    inner_feature, inner_threshold, leaf = arrays
    return RegressionForest(inner_feature=inner_feature, inner_threshold=inner_threshold, leaf=leaf,
                            depth=int(np.log2(leaf.shape[1])))
