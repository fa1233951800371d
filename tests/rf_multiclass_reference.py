"""Test-side restatement of MLlib 2.1's RandomForest.trainClassifier for C
classes (the oracle module is frozen and binary; this adds the class axis).

Thresholds, bins and the invalid-gain marker are the oracle's
(oracle.rf_oracle: num_splits, find_splits, bin_values, INVALID_GAIN); what
depends on the labels is restated here with C classes wherever the oracle has
two:

  impurity Gini.calculate: total = sum of the counts; impurity = 1; for each
           class in class order: f = c / total; impurity -= f * f (0 when
           total == 0)
  gain     calculateImpurityStats: invalid when a child's count <
           minInstancesPerNode; gain = impurity - (lc/tc) * imp_l - (rc/tc) *
           imp_r; invalid when gain < minInfoGain
  best     first maximum over the node's features in subset order, then the
           feature's splits in index order
  growth   leaf when gain <= 0 or at maxDepth; a child is created as a leaf
           when it reaches maxDepth or its impurity is 0.0
  predict  indexOfLargestArrayElement: the first index of the largest count

The bagging weights and the per-node feature subsets are inputs, as in the
oracle, so the GPU trainer is compared on identical draws.
"""
import numpy as np

from oracle.rf_oracle import INVALID_GAIN, bin_values, find_splits, num_splits

POS_INF_BITS = int(np.array([np.inf], dtype=np.float32).view(np.int32)[0])


def gini(counts) -> float:
    total = float(sum(int(c) for c in counts))
    if total == 0:
        return 0.0
    imp = 1.0
    for c in counts:
        f = float(c) / total
        imp -= f * f
    return imp


def impurity_stats(left, right, parent_impurity: float, min_instances: int = 1, min_info_gain: float = 0.0):
    """calculateImpurityStats -> (gain, left impurity, right impurity)."""
    lc = int(sum(int(c) for c in left))
    rc = int(sum(int(c) for c in right))
    if lc < min_instances or rc < min_instances:
        return INVALID_GAIN, None, None
    tc = lc + rc
    li, ri = gini(left), gini(right)
    lw = lc / float(tc)
    rw = rc / float(tc)
    gain = parent_impurity - lw * li - rw * ri
    if gain < min_info_gain:
        return INVALID_GAIN, None, None
    return gain, li, ri


def predict(counts) -> int:
    """indexOfLargestArrayElement (strict >: first maximum)."""
    best = 0
    for c in range(1, len(counts)):
        if counts[c] > counts[best]:
            best = c
    return best


def train_tree(bins, labels, weights, subsets, n_splits_f, max_depth, n_classes, min_instances=1,
               min_info_gain=0.0):
    """One tree; arguments and result as oracle.rf_oracle.train_tree, labels
    class ids in [0, n_classes)."""
    C = int(n_classes)
    n_inner = (1 << max_depth) - 1
    split_feature = np.full(n_inner, -1, dtype=np.int64)
    split_bin = np.zeros(n_inner, dtype=np.int64)
    leaf_class = np.zeros(1 << max_depth, dtype=np.uint8)
    labels = np.asarray(labels, dtype=np.int64)
    weights = np.asarray(weights, dtype=np.int64)
    node = np.zeros(bins.shape[0], dtype=np.int64)
    level_nodes = {0: False}  # heap index -> preset leaf flag
    for level in range(max_depth + 1):
        nxt = {}
        for h, preset_leaf in sorted(level_nodes.items()):
            rows = np.nonzero((node == h) & (weights > 0))[0]
            cnt = np.bincount(labels[rows], weights=weights[rows], minlength=C).astype(np.int64)
            best_gain, best = INVALID_GAIN, None
            if not preset_leaf and level < max_depth:
                parent_imp = gini(cnt)
                for f in subsets[h]:
                    f = int(f)
                    ns = int(n_splits_f[f])
                    hist = np.zeros((ns + 1, C), dtype=np.int64)
                    np.add.at(hist, (bins[rows, f], labels[rows]), weights[rows])
                    cum = np.cumsum(hist, axis=0)
                    for k in range(ns):
                        left = cum[k]
                        gain, li, ri = impurity_stats(left, cnt - left, parent_imp, min_instances, min_info_gain)
                        if gain > best_gain:
                            best_gain, best = gain, (f, k, li, ri)
            if preset_leaf or level == max_depth or best_gain <= 0:
                span = 1 << (max_depth - level)
                first = (h + 1) * span - 1 - n_inner
                leaf_class[first:first + span] = predict(cnt)
                continue
            f, k, li, ri = best
            split_feature[h] = f
            split_bin[h] = k
            child_leaf = level + 1 == max_depth
            nxt[2 * h + 1] = child_leaf or li == 0.0
            nxt[2 * h + 2] = child_leaf or ri == 0.0
            go_right = bins[:, f] > k
            here = node == h
            node[here & ~go_right] = 2 * h + 1
            node[here & go_right] = 2 * h + 2
        level_nodes = nxt
        if not level_nodes:
            break
    return split_feature, split_bin, leaf_class


def train_classifier(X, y, weights, subsets, n_classes, max_depth=4, max_bins=32, split_rows=None,
                     min_instances=1, min_info_gain=0.0):
    """As oracle.rf_oracle.train_classifier with numClasses = n_classes:
    (thresholds per feature, split_feature [T, n_inner], split_threshold fp64
    [T, n_inner] (NaN where no split), leaf_class [T, n_leaf])."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    ns = num_splits(n, max_bins)
    sample = X if split_rows is None else X[np.asarray(split_rows)]
    thresholds = [find_splits(sample[:, f], ns) for f in range(d)]
    n_splits_f = np.array([t.size for t in thresholds], dtype=np.int64)
    bins = np.stack([bin_values(X[:, f], thresholds[f]) for f in range(d)], axis=1)
    T = weights.shape[0]
    n_inner = (1 << max_depth) - 1
    sf = np.full((T, n_inner), -1, dtype=np.int64)
    st = np.full((T, n_inner), np.nan)
    lc = np.zeros((T, 1 << max_depth), dtype=np.uint8)
    for t in range(T):
        f_, b_, l_ = train_tree(bins, y, weights[t], subsets[t], n_splits_f, max_depth, n_classes, min_instances,
                                min_info_gain)
        sf[t], lc[t] = f_, l_
        for h in np.nonzero(f_ >= 0)[0]:
            st[t, h] = thresholds[f_[h]][b_[h]]
    return thresholds, sf, st, lc


def heap_arrays(sf, st, lc):
    """(inner int32 [T, n_inner, 2], leaf uint8 [T, n_leaf]) in the device heap
    layout: (feature, fp32 threshold bits), (0, +inf) where there is no split.
    The thresholds are fp32 pool values, so the cast is exact."""
    inner = np.zeros(sf.shape + (2,), dtype=np.int32)
    inner[..., 1] = POS_INF_BITS
    m = sf >= 0
    inner[..., 0][m] = sf[m]
    inner[..., 1][m] = st[m].astype(np.float32).view(np.int32)
    return inner, lc


def heap_forest(sf, st, lc, n_classes, classes_=None):
    """The trained heap arrays as a dal.forest.Forest of n_classes."""
    from dal.forest import Forest

    inner, leaf = heap_arrays(sf, st, lc)
    depth = int(np.log2(leaf.shape[1]))
    return Forest(inner=inner, leaf=leaf, depth=depth, n_classes=int(n_classes),
                  classes_=None if classes_ is None else np.asarray(classes_))


class ReferenceModel:
    """A reference-trained forest with ``predict`` (labels by majority of the
    trees' hard votes, ties to the lowest class id), for the loop test."""

    def __init__(self, forest):
        self.forest = forest

    def predict(self, X):
        import multiclass_reference as M

        ids = M.pred(M.counts(self.forest, X))
        return ids if self.forest.classes_ is None else self.forest.classes_[ids]


def loop_trainer(classes, n_classes, max_depth=4):
    """A run_loop trainer callable (X, y, T, seed) -> ReferenceModel making
    the draws dal.random_forest.train_classifier makes for that seed."""
    from dal.random_forest import bagging_inputs

    classes = np.asarray(classes)

    def fit(X, y, T, seed):
        ids = np.searchsorted(classes, np.asarray(y))
        w, s = bagging_inputs(X.shape[0], X.shape[1], T, max_depth, seed)
        _, sf, st, lc = train_classifier(X, ids, w, s, n_classes, max_depth=max_depth)
        return ReferenceModel(heap_forest(sf, st, lc, n_classes, classes))

    return fit
