"""GPU random-forest training: the drop-in for MLlib's
``RandomForest.trainClassifier`` on the AL loop's labeled set (SURVEY §8(f)
row 4).

Reference call sites (the per-iteration model fit):
  final_thesis/uncertainty_sampling.py:71-76
  final_thesis/density_weighting.py:119-124
      model = RandomForest.trainClassifier(train, numClasses=2,
                  categoricalFeaturesInfo={}, numTrees=T,
                  featureSubsetStrategy="auto", impurity='gini')   # maxDepth=4, maxBins=32

Every arithmetic step runs in libdal (csrc/rf_train.hip): threshold search
(findSplitsForContinuousFeature), binning, level-wise weighted Gini histograms
and split selection.  The host draws what MLlib draws from its JVM RNGs --
the Poisson(1) bootstrap weights and the per-node feature subsets -- with
numpy (seeded), so a fit is deterministic; the oracle (oracle/rf_oracle.py)
takes the same draws.  The result is a ``dal.forest.Forest`` in the heap
layout the selection kernels consume, already resident on the device.

``num_classes`` > 2 (MLlib's numClasses) takes the C-class level kernels of
csrc/rf_train_multi.hip (dal_rf_train_multiclass): up to DAL_MC_MAX_CLASSES
classes and DAL_MC_MAX_TREES trees; the binary path is untouched.

``train_regressor`` is MLlib's ``RandomForest.trainRegressor`` (variance
impurity; the LAL model of lal_direct_mllib_implementation/classes/
active_learner.py:354-363) through csrc/rf_train_regress.hip: the same growth
with exact variance sums (include/dal.h), fp32 or fp64 rows and fp64
thresholds, into a ``dal.forest.RegressionForest``.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

from . import _lib
from ._lib import (DAL_FLAG_RF_SPLITS, DAL_MC_MAX_CLASSES, DAL_MC_MAX_TREES, DAL_RF_MAX_DEPTH,
                   DAL_RF_MAX_SPLIT_SAMPLE, DAL_RF_MAX_SPLIT_SAMPLE_F64, DAL_RF_MAX_SPLITS, DAL_RF_REG_MAX_LIMBS,
                   DAL_RF_SPLIT_LDS_BYTES, call)
from .forest import Forest, RegressionForest


def feature_subset_size(n_features: int, n_trees: int, strategy: str = "auto") -> int:
    """MLlib featureSubsetStrategy: "auto" = "all" for one tree, "sqrt" for a
    forest (classification); also "all", "sqrt", "log2", "onethird"."""
    if strategy == "auto":
        strategy = "all" if n_trees == 1 else "sqrt"
    if strategy == "all":
        return n_features
    if strategy == "sqrt":
        return int(math.ceil(math.sqrt(n_features)))
    if strategy == "log2":
        return max(1, int(math.ceil(math.log2(n_features))))
    if strategy == "onethird":
        return int(math.ceil(n_features / 3.0))
    raise ValueError(f"unknown featureSubsetStrategy {strategy!r}")


def bagging_inputs(n: int, d: int, n_trees: int, max_depth: int = 4, seed: int = 0,
                   feature_subset_strategy: str = "auto"):
    """(weights int32 [T, n], subsets int32 [T, 2^max_depth - 1, m]): Poisson(1)
    instance weights per tree (BaggedPoint with replacement when T > 1, all
    ones for a single tree) and the feature subset of every heap node (a
    random m-subset in draw order; all features in index order when m = d)."""
    rng = np.random.default_rng(seed)
    m = feature_subset_size(d, n_trees, feature_subset_strategy)
    if n_trees > 1:
        weights = rng.poisson(1.0, size=(n_trees, n)).astype(np.int32)
    else:
        weights = np.ones((1, n), dtype=np.int32)
    n_inner = (1 << max_depth) - 1
    if m == d:
        subsets = np.broadcast_to(np.arange(d, dtype=np.int32), (n_trees, n_inner, d)).copy()
    else:
        keys = rng.random((n_trees, n_inner, d))
        subsets = np.argsort(keys, axis=2, kind="stable")[:, :, :m].astype(np.int32)
    return weights, subsets


def split_sample_rows(n: int, max_bins: int = 32, seed: int = 0):
    """Rows the thresholds are fitted on.  MLlib uses every row when
    n <= max(maxBins^2, 10000), else a Bernoulli sample of expected size
    10000 (DecisionTree findSplits; its RNG differs, so parity is unpinned
    for that case).  None = all rows."""
    required = max(max_bins * max_bins, 10000)
    if n <= required and n <= DAL_RF_MAX_SPLIT_SAMPLE:
        return None
    rng = np.random.default_rng(seed + 0x5EED)
    rows = np.nonzero(rng.random(n) < min(required, DAL_RF_MAX_SPLIT_SAMPLE) / float(n))[0]
    return rows[:DAL_RF_MAX_SPLIT_SAMPLE].astype(np.int64)


def num_splits(n: int, max_bins: int = 32) -> int:
    """DecisionTreeMetadata: numBins = min(maxBins, numExamples), numSplits = numBins - 1."""
    return min(int(max_bins), int(n)) - 1


def _stream(device):
    import torch

    return torch.cuda.current_stream(device).cuda_stream


def check_labels(y, n: int, num_classes: int = 2, num_trees=None) -> np.ndarray:
    """The labels as n class-id bytes, or ValueError: ids lie in
    [0, num_classes), 2 <= num_classes <= DAL_MC_MAX_CLASSES, and a forest of
    more than two classes has at most DAL_MC_MAX_TREES trees (the multiclass
    score kernels take no more).  Pure host code: needs no device."""
    num_classes = int(num_classes)
    if not 2 <= num_classes <= DAL_MC_MAX_CLASSES:
        raise ValueError(f"num_classes must lie in [2, {DAL_MC_MAX_CLASSES}], not {num_classes}")
    if num_classes > 2 and num_trees is not None and not 1 <= int(num_trees) <= DAL_MC_MAX_TREES:
        raise ValueError(f"a forest of {num_classes} classes has 1..{DAL_MC_MAX_TREES} trees, not {num_trees}")
    yv = np.asarray(y).reshape(-1)
    if num_classes == 2:
        if yv.shape[0] != n or not np.isin(yv, (0, 1)).all():
            raise ValueError("labels must be n values in {0, 1}")
    elif yv.shape[0] != n or not np.isin(yv, np.arange(num_classes)).all():
        raise ValueError(f"labels must be n class ids in [0, {num_classes})")
    return yv.astype(np.uint8)


def check_split_histogram(m: int, n_splits: int, n_classes: int = 2) -> None:
    """The split kernel (dal_rf_train, dal_rf_train_multiclass) holds one
    node's (feature slot, bin, class) histogram in LDS: m * (n_splits + 2) *
    n_classes int32 counts must fit DAL_RF_SPLIT_LDS_BYTES.  MLlib itself has
    no such limit; raise a clear error instead of the kernel's
    DAL_ERR_UNSUPPORTED."""
    need = int(m) * (int(n_splits) + 2) * int(n_classes) * 4
    if need > DAL_RF_SPLIT_LDS_BYTES:
        raise ValueError(f"{m} candidate features per node x {n_splits + 1} thresholds need {need} bytes of "
                         f"split histogram, more than the GPU trainer's {DAL_RF_SPLIT_LDS_BYTES} "
                         "(lower max_bins or use a smaller feature subset)")


# ------------------------------------------- host preparation, shared with
# the row-sharded fits of dal.parallel (n is then the size of the whole
# training set and the labels are the rank's own)
def check_growth(max_depth: int, max_bins: int) -> None:
    if not 1 <= max_depth <= DAL_RF_MAX_DEPTH:
        raise ValueError(f"max_depth must lie in [1, {DAL_RF_MAX_DEPTH}]")
    if not 2 <= max_bins <= DAL_RF_MAX_SPLITS:
        raise ValueError(f"max_bins must lie in [2, {DAL_RF_MAX_SPLITS}]")


def classifier_inputs(n: int, d: int, y, n_labels: int, num_trees: int, max_depth: int, max_bins: int, seed: int,
                      feature_subset_strategy: str, weights, feature_subsets, num_classes: int,
                      check_weights: bool = False):
    """What train_classifier settles on the host before any device call, in
    its order and with its messages: the growth limits, the ``n_labels``
    labels as class-id bytes, the seeded draws (or the caller's) as int32
    arrays over the n rows, their shapes, numSplits, the split kernel's LDS
    limit and the rows the thresholds are fitted on.  ``y`` None: no labels
    here (their count limits alone are checked)."""
    check_growth(max_depth, max_bins)
    if y is None:  # a sharded fit: every rank has checked its own labels
        y, n_labels = np.zeros(0, dtype=np.uint8), 0
    labels = check_labels(y, n_labels, num_classes)
    if weights is None or feature_subsets is None:
        w_draw, s_draw = bagging_inputs(n, d, num_trees, max_depth, seed, feature_subset_strategy)
        weights = w_draw if weights is None else weights
        feature_subsets = s_draw if feature_subsets is None else feature_subsets
    w = check_tree_weights(weights) if check_weights else np.ascontiguousarray(weights, dtype=np.int32)
    sub = np.ascontiguousarray(feature_subsets, dtype=np.int32)
    T = int(w.shape[0])
    n_inner = (1 << max_depth) - 1
    if w.ndim != 2 or tuple(w.shape) != (T, n) or sub.ndim != 3 or tuple(sub.shape[:2]) != (T, n_inner):
        raise ValueError(f"weights must be [T, {n}] and feature_subsets [T, {n_inner}, m]")
    m = int(sub.shape[2])
    if not 1 <= m <= d:
        raise ValueError("feature subsets must hold 1..d features")
    ns = num_splits(n, max_bins)
    check_split_histogram(m, ns, num_classes)
    check_labels(y, n_labels, num_classes, num_trees=T)
    return SimpleNamespace(labels=labels, weights=w, subsets=sub, T=T, m=m, ns=ns, n_inner=n_inner,
                           num_classes=int(num_classes), rows=split_sample_rows(n, max_bins, seed))


def device_rows(X, dev, keep_f64: bool = False):
    """The training rows as a contiguous device tensor: fp32, or fp64 where
    the regressor is given fp64 rows (they train unrounded)."""
    import torch

    if isinstance(X, torch.Tensor):
        x = X.to(dev) if keep_f64 and X.dtype == torch.float64 else X.to(device=dev, dtype=torch.float32)
    else:
        xs = np.asarray(X)
        host_dtype = np.float64 if keep_f64 and xs.dtype == np.float64 else np.float32
        x = torch.from_numpy(np.ascontiguousarray(xs, dtype=host_dtype)).to(dev)
    return x.contiguous()


def device_find_splits(x, rows, ns: int, f64_thresholds: bool):
    """dal_rf_find_splits (fp32 thresholds, the classifiers) or
    dal_rf_find_splits_f64 (fp64 thresholds, the regressor) over the sample
    ``rows`` of x (None: every row): (thresholds [d, 255], n_splits [d],
    status [1]) on x's device, stream-ordered."""
    import torch

    dev = x.device
    n, d = int(x.shape[0]), int(x.shape[1])
    n_sample = n if rows is None else int(rows.shape[0])
    rows_t = None if rows is None else torch.from_numpy(rows).to(dev)
    thresholds = torch.empty((d, DAL_RF_MAX_SPLITS), dtype=torch.float64 if f64_thresholds else torch.float32,
                             device=dev)
    n_splits = torch.empty(d, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rows_p = 0 if rows_t is None else rows_t.data_ptr()
    if f64_thresholds:
        x_dtype = _lib.DAL_X_F64 if x.dtype == torch.float64 else _lib.DAL_X_F32
        call("dal_rf_find_splits_f64", x.data_ptr(), x_dtype, n, d, d, rows_p, n_sample, ns, thresholds.data_ptr(),
             n_splits.data_ptr(), status.data_ptr(), _stream(dev))
    else:
        call("dal_rf_find_splits", x.data_ptr(), n, d, d, rows_p, n_sample, ns, thresholds.data_ptr(),
             n_splits.data_ptr(), status.data_ptr(), _stream(dev))
    return thresholds, n_splits, status


def _workspace(nbytes: int, dev):
    """(tensor, 256-B aligned address) of nbytes of device scratch."""
    import torch

    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    return ws, (ws.data_ptr() + 255) // 256 * 256


def check_split_overflow(status) -> None:
    if int(status) & DAL_FLAG_RF_SPLITS:
        raise _lib.DalError("threshold search emitted more than num_splits + 1 thresholds")


def classifier_forest(inner, leaf, max_depth: int, num_classes: int, thresholds, n_splits) -> Forest:
    """The Forest of the trained heap arrays; device tensors stay resident."""
    on_dev = hasattr(inner, "is_cuda") and inner.is_cuda
    forest = Forest(inner=_host(inner), leaf=_host(leaf), depth=max_depth, n_classes=int(num_classes))
    if on_dev:
        forest._dev[str(inner.device)] = (inner, leaf)
    forest.split_thresholds = (thresholds, n_splits)
    return forest


def _host(t) -> np.ndarray:
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def train_classifier(X, y, num_trees: int = 10, max_depth: int = 4, max_bins: int = 32, seed: int = 0,
                     feature_subset_strategy: str = "auto", weights=None, feature_subsets=None,
                     min_instances_per_node: int = 1, min_info_gain: float = 0.0, device=None,
                     num_classes: int = 2) -> Forest:
    """RandomForest.trainClassifier(numClasses=num_classes,
    categoricalFeaturesInfo={}, impurity='gini') on the GPU.  X [n, d] (numpy
    or torch), y labels in {0,1}.  ``weights`` [T, n] / ``feature_subsets``
    [T, 2^max_depth - 1, m] override the seeded draws (bagging_inputs).
    num_classes > 2 (dal_rf_train_multiclass, csrc/rf_train_multi.hip): y holds
    class ids in [0, num_classes), at most DAL_MC_MAX_CLASSES classes and
    DAL_MC_MAX_TREES trees, and the result is a Forest of n_classes =
    num_classes for the multiclass score kernels."""
    import torch

    from .engine import _require_cuda

    dev = _require_cuda(device)
    lib = _lib.load()
    x = device_rows(X, dev)
    if x.dim() != 2 or x.shape[0] < 1:
        raise ValueError("training set must be a non-empty 2-D [rows, features] array")
    n, d = int(x.shape[0]), int(x.shape[1])
    yv = y.cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
    p = classifier_inputs(n, d, yv, n, num_trees, max_depth, max_bins, seed, feature_subset_strategy, weights,
                          feature_subsets, num_classes)
    labels = torch.from_numpy(p.labels).to(dev)
    w = torch.from_numpy(p.weights).to(dev)
    sub = torch.from_numpy(p.subsets).to(dev)
    T, m, ns, n_inner = p.T, p.m, p.ns, p.n_inner
    thresholds, n_splits, status = device_find_splits(x, p.rows, ns, f64_thresholds=False)
    s = _stream(dev)
    multi = int(num_classes) > 2
    wsb = int(lib.dal_rf_train_multiclass_workspace_bytes(n, d, T, max_depth, m, ns, int(num_classes))) if multi \
        else int(lib.dal_rf_train_workspace_bytes(n, d, T, max_depth, m, ns))
    ws, wsp = _workspace(wsb, dev)
    inner = torch.empty((T, n_inner, 2), dtype=torch.int32, device=dev)
    leaf = torch.empty((T, n_inner + 1), dtype=torch.uint8, device=dev)
    head = (x.data_ptr(), n, d, d, labels.data_ptr(), thresholds.data_ptr(), n_splits.data_ptr(), ns,
            w.data_ptr(), sub.data_ptr(), m, T, max_depth, int(min_instances_per_node), float(min_info_gain))
    tail = (inner.data_ptr(), leaf.data_ptr(), wsp, wsb, s)
    if multi:
        call("dal_rf_train_multiclass", *head, int(num_classes), *tail)
    else:
        call("dal_rf_train", *head, *tail)
    check_split_overflow(status.item())
    return classifier_forest(inner, leaf, max_depth, num_classes, thresholds, n_splits)


# ---------------------------------------------------------------- regression
LIMB_BITS = 31  # csrc/rf_exact_sum.hpp


def regression_subset_strategy(n_trees: int, strategy: str = "auto") -> str:
    """featureSubsetStrategy of trainRegressor: "auto" is "all" for one tree
    and "onethird" for a forest; every other name stands for itself."""
    if strategy == "auto":
        return "all" if n_trees == 1 else "onethird"
    return strategy


def regression_subset_size(n_features: int, n_trees: int, strategy: str = "auto") -> int:
    """Features per node of a regression forest: ceil(d / 3) for "auto" with
    more than one tree, d for one tree; the other names as feature_subset_size."""
    return feature_subset_size(n_features, n_trees, regression_subset_strategy(n_trees, strategy))


NO_BITS = (2 ** 31 - 1, -(2 ** 31))  # (low, top) of values without a set bit: neutral under MIN / MAX


def exact_sum_bounds(values):
    """(low, top) of a vector of finite doubles: the exponent of the lowest
    set bit over the nonzero values and the exponent above the highest set
    bit; NO_BITS when there is no nonzero value (an empty or all-zero shard
    of a sharded fit then leaves the other shards' format alone)."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    v = v[v != 0.0]
    if v.size == 0:
        return NO_BITS
    mant, exp = np.frexp(v)  # |mant| in [0.5, 1): the highest set bit has exponent exp - 1
    m = np.abs(mant * 9007199254740992.0).astype(np.int64)  # 53-bit integers, exact
    low_bit = m & -m
    tz = np.log2(low_bit.astype(np.float64)).astype(np.int64)  # powers of two: exact
    return int((exp.astype(np.int64) - 53 + tz).min()), int(exp.max())


def format_from_bounds(low: int, top: int):
    """(Q, K, span) of the exact accumulator from (low, top): (0, 1, 0) for NO_BITS."""
    if (int(low), int(top)) == NO_BITS:
        return 0, 1, 0
    span = int(top) - int(low)
    return int(low), max(1, -(-span // LIMB_BITS)), span


def exact_sum_format(values):
    """(Q, K, span) of a vector of finite doubles for the exact accumulator
    (csrc/rf_exact_sum.hpp): Q the exponent of the lowest set bit over the
    nonzero values, span = (the exponent above the highest set bit) - Q, K =
    max(1, ceil(span / 31)) limbs.  (0, 1, 0) when every value is zero."""
    return format_from_bounds(*exact_sum_bounds(values))


def regression_label_bounds(y, n: int):
    """The labels as n finite doubles with exact_sum_bounds of y and of
    fl(y * y), or ValueError.  Pure host code."""
    yv = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
    if yv.shape[0] != n:
        raise ValueError(f"labels must be {n} values, one per row")
    if not np.isfinite(yv).all():
        raise ValueError("labels must be finite")
    with np.errstate(over="ignore"):
        sq = yv * yv
    if not np.isfinite(sq).all():
        raise ValueError("a label's square overflows fp64")
    return yv, exact_sum_bounds(yv), exact_sum_bounds(sq)


def regression_formats(bounds_y, bounds_sq):
    """((Q, K) of y, (Q, K) of fl(y * y)) from their (low, top), within the
    exact variance sums' limits, or ValueError."""
    fmt = []
    for what, b in (("labels", bounds_y), ("squared labels", bounds_sq)):
        q, k, span = format_from_bounds(*b)
        if k > DAL_RF_REG_MAX_LIMBS:
            raise ValueError(f"the {what} span {span} bits between their highest and lowest set bit, more than the "
                             f"{DAL_RF_REG_MAX_LIMBS * LIMB_BITS} the exact variance sums hold")
        if q + span + LIMB_BITS > 1023:
            raise ValueError(f"a weighted sum of the {what} could overflow fp64")
        fmt.append((q, k))
    return fmt[0], fmt[1]


def check_regression_labels(y, n: int):
    """The labels as n finite doubles and the two accumulator formats
    ((Q, K) of y, (Q, K) of fl(y * y)), or ValueError.  Pure host code."""
    yv, b_y, b_sq = regression_label_bounds(y, n)
    f_y, f_sq = regression_formats(b_y, b_sq)
    return yv, f_y, f_sq


def check_tree_weights(weights) -> np.ndarray:
    """Bagging weights as int32 [T, n] >= 0 whose per-tree sums stay below
    2^31 (the exact sums' 64-bit words cannot overflow then), or ValueError."""
    w = np.asarray(weights)
    if w.ndim != 2 or (w.size and w.min() < 0):
        raise ValueError("weights must be a non-negative [T, n] array")
    tot = w.sum(axis=1, dtype=np.int64)
    if tot.size and int(tot.max()) >= 1 << 31:
        raise ValueError(f"a tree's weights sum to {int(tot.max())}: the GPU trainer needs less than 2^31")
    return np.ascontiguousarray(w, dtype=np.int32)


def regression_split_sample_rows(n: int, max_bins: int, seed: int, f64: bool):
    """split_sample_rows with the row limit of the fp64 threshold search."""
    cap = DAL_RF_MAX_SPLIT_SAMPLE_F64 if f64 else DAL_RF_MAX_SPLIT_SAMPLE
    required = max(max_bins * max_bins, 10000)
    if n <= required and n <= cap:
        return None
    rng = np.random.default_rng(seed + 0x5EED)
    rows = np.nonzero(rng.random(n) < min(required, cap) / float(n))[0]
    return rows[:cap].astype(np.int64)


def regressor_inputs(n: int, d: int, num_trees: int, max_depth: int, max_bins: int, seed: int,
                     feature_subset_strategy: str, weights, feature_subsets, k_y: int, k_sq: int):
    """What train_regressor settles on the host after the labels, in its
    order and with its messages: the seeded draws (or the caller's) over the n
    rows, check_tree_weights, the shapes, numSplits and the split kernel's LDS
    limit.  Shared with dal.parallel (n = the whole training set)."""
    if weights is None or feature_subsets is None:
        w_draw, s_draw = bagging_inputs(n, d, num_trees, max_depth, seed,
                                        regression_subset_strategy(num_trees, feature_subset_strategy))
        weights = w_draw if weights is None else weights
        feature_subsets = s_draw if feature_subsets is None else feature_subsets
    w_np = check_tree_weights(weights)
    sub_np = np.ascontiguousarray(feature_subsets, dtype=np.int32)
    T = int(w_np.shape[0])
    n_inner = (1 << max_depth) - 1
    if T < 1 or w_np.shape != (T, n) or sub_np.ndim != 3 or sub_np.shape[:2] != (T, n_inner):
        raise ValueError(f"weights must be [T, {n}] and feature_subsets [T, {n_inner}, m]")
    m = int(sub_np.shape[2])
    if not 1 <= m <= d or sub_np.min() < 0 or sub_np.max() >= d:
        raise ValueError("feature subsets must hold 1..d features in [0, d)")
    ns = num_splits(n, max_bins)
    W = 1 + k_y + k_sq
    need = m * (ns + 2) * W * 8
    if need > DAL_RF_SPLIT_LDS_BYTES:
        raise ValueError(f"{m} candidate features per node x {ns + 1} thresholds x {W} words need {need} bytes of "
                         f"split histogram, more than the GPU trainer's {DAL_RF_SPLIT_LDS_BYTES} "
                         "(lower max_bins or use a smaller feature subset)")
    return SimpleNamespace(weights=w_np, subsets=sub_np, T=T, m=m, ns=ns, n_inner=n_inner)


def regressor_tree_chunk(tree_chunk, n: int, T: int, max_depth: int, m: int, ns: int, k_y: int, k_sq: int) -> int:
    """Trees per launch: the caller's, or what keeps the workspace at about 256 MiB."""
    if tree_chunk is None:
        per_tree = int(_lib.load().dal_rf_train_regressor_workspace_bytes(n, 1, max_depth, m, ns, k_y, k_sq)) + 4 * n
        tree_chunk = max(1, (256 << 20) // per_tree)
    return max(1, min(int(tree_chunk), T))


def regression_forest(feat, thr, leaf, max_depth: int, thresholds, n_splits) -> RegressionForest:
    """The RegressionForest of the trained heap arrays; device tensors stay resident."""
    on_dev = hasattr(feat, "is_cuda") and feat.is_cuda
    model = RegressionForest(inner_feature=_host(feat), inner_threshold=_host(thr), leaf=_host(leaf),
                             depth=max_depth)
    if on_dev:
        model._dev[str(feat.device)] = (feat, thr, leaf)
    model.split_thresholds = (thresholds, n_splits)
    return model


def train_regressor(X, y, num_trees: int = 10, max_depth: int = 4, max_bins: int = 32, seed: int = 0,
                    feature_subset_strategy: str = "auto", weights=None, feature_subsets=None,
                    min_instances_per_node: int = 1, min_info_gain: float = 0.0, device=None,
                    tree_chunk=None) -> RegressionForest:
    """RandomForest.trainRegressor(categoricalFeaturesInfo={},
    impurity="variance") on the GPU (csrc/rf_train_regress.hip): X [n, d] fp32
    or fp64 (numpy or torch; fp64 rows train unrounded), y [n] real labels.
    ``weights`` [T, n] / ``feature_subsets`` [T, 2^max_depth - 1, m] override
    the seeded draws (bagging_inputs with regression's "auto" = onethird).
    The variance sums are exact (include/dal.h), so the result is the same
    bytes on every run and for every ``tree_chunk`` (trees per launch; None
    bounds the workspace at about 256 MiB).  The RegressionForest is resident
    on the device; ``split_thresholds`` holds (thresholds fp64 [d, 255],
    n_splits int32 [d]) there."""
    import torch

    xs = X if isinstance(X, torch.Tensor) else np.asarray(X)
    if xs.ndim != 2 or xs.shape[0] < 1 or xs.shape[1] < 1:
        raise ValueError("training set must be a non-empty 2-D [rows, features] array")
    n, d = int(xs.shape[0]), int(xs.shape[1])
    check_growth(max_depth, max_bins)
    yv, (q_y, k_y), (q_sq, k_sq) = check_regression_labels(y.cpu().numpy() if isinstance(y, torch.Tensor) else y, n)
    p = regressor_inputs(n, d, num_trees, max_depth, max_bins, seed, feature_subset_strategy, weights,
                         feature_subsets, k_y, k_sq)
    w_np, sub_np, T, m, ns, n_inner = p.weights, p.subsets, p.T, p.m, p.ns, p.n_inner

    from .engine import _require_cuda

    dev = _require_cuda(device)
    lib = _lib.load()
    x = device_rows(xs, dev, keep_f64=True)
    f64 = x.dtype == torch.float64
    x_dtype = _lib.DAL_X_F64 if f64 else _lib.DAL_X_F32
    rows = regression_split_sample_rows(n, max_bins, seed, f64)
    thresholds, n_splits, status = device_find_splits(x, rows, ns, f64_thresholds=True)
    bins = torch.empty((n, d), dtype=torch.uint8, device=dev)
    s = _stream(dev)
    call("dal_rf_bin_rows", x.data_ptr(), x_dtype, n, d, d, thresholds.data_ptr(), n_splits.data_ptr(),
         bins.data_ptr(), s)
    y_t = torch.from_numpy(yv).to(dev)
    tree_chunk = regressor_tree_chunk(tree_chunk, n, T, max_depth, m, ns, k_y, k_sq)
    wsb = int(lib.dal_rf_train_regressor_workspace_bytes(n, tree_chunk, max_depth, m, ns, k_y, k_sq))
    ws, wsp = _workspace(wsb, dev)
    feat = torch.empty((T, n_inner), dtype=torch.int32, device=dev)
    thr = torch.empty((T, n_inner), dtype=torch.float64, device=dev)
    leaf = torch.empty((T, n_inner + 1), dtype=torch.float64, device=dev)
    for t0 in range(0, T, tree_chunk):
        t1 = min(T, t0 + tree_chunk)
        w_t = torch.from_numpy(w_np[t0:t1]).to(dev)
        sub_t = torch.from_numpy(sub_np[t0:t1]).to(dev)
        call("dal_rf_train_regressor", bins.data_ptr(), n, d, y_t.data_ptr(), thresholds.data_ptr(),
             n_splits.data_ptr(), ns, w_t.data_ptr(), sub_t.data_ptr(), m, t1 - t0, max_depth,
             int(min_instances_per_node), float(min_info_gain), q_y, k_y, q_sq, k_sq, feat[t0:t1].data_ptr(),
             thr[t0:t1].data_ptr(), leaf[t0:t1].data_ptr(), wsp, wsb, s)
    check_split_overflow(status.item())
    return regression_forest(feat, thr, leaf, max_depth, thresholds, n_splits)


def predict(forest: Forest, X, device=None):
    """RandomForestModel.predict (majority vote of the trees' hard labels;
    ties -> class 0) on the GPU: (labels uint8 [n], votes int32 [n]).  A
    multiclass forest (n_classes > 2) returns (pred uint8 [n], counts uint8
    [n, C]): pred is the class id with the most trees, ties to the lowest id
    (``forest.classes_[pred]`` is the label where the forest carries labels).
    A ProbabilityForest returns (pred uint8 [n], sums int64 [n, C]): pred is
    the class of the largest averaged probability (scikit-learn's
    ``rf.predict``), ties to the lowest id; predict_proba gives the
    probabilities."""
    import torch

    from . import engine
    from ._lib import DAL_ASCENDING, DAL_MC_LEAST_CONFIDENCE
    from .forest import ProbabilityForest

    state = X if isinstance(X, engine.PoolState) else engine.PoolState(X, device=device)
    if isinstance(forest, ProbabilityForest):
        sums, pred, _, _ = engine.forest_score_soft(state, forest, None, DAL_ASCENDING,
                                                    engine.SOFT_KINDS["least_confidence"])
        return pred, sums
    if forest.n_classes > 2:
        lut = engine.device_multiclass_lut("least_confidence", forest.n_trees, state.device)
        counts, pred, _, _ = engine.forest_score_multiclass(state, forest, lut, None, DAL_ASCENDING,
                                                            DAL_MC_LEAST_CONFIDENCE)
        return pred, counts
    lut = engine.device_lut("least_confidence", forest.n_trees, state.device)
    votes, _, _, _ = engine.forest_score(state, forest, lut, state.flags, DAL_ASCENDING)
    return (2 * votes > forest.n_trees).to(torch.uint8), votes


def predict_proba(forest, X, device=None):
    """scikit-learn's ``RandomForestClassifier.predict_proba`` of a
    ProbabilityForest on the GPU: (proba fp64 [n, C], pred uint8 [n]).
    proba[i, c] = (double)S_c / (double)(T 2^31), the exact class sums of the
    quantised leaf distributions over one IEEE division: within 2^-31 of
    ``rf.predict_proba``; pred is the lowest class of the largest sum."""
    from .engine import soft_proba
    from .forest import ProbabilityForest

    if not isinstance(forest, ProbabilityForest):
        raise ValueError("predict_proba needs a dal.forest.ProbabilityForest (a Forest keeps no leaf distributions)")
    pred, sums = predict(forest, X, device=device)
    return soft_proba(sums, forest.denominator), pred


def predict_regression(model, X, device=None):
    """RandomForestModel.predict of a regression model (MLlib's
    ``trees.map(predict).sum / numTrees``, active_learner.py:319) on the GPU:
    fp64 [n], sequential fp64 sum in tree order.  ``model``: a
    dal.forest.RegressionForest; X: a PoolState, or an fp32 or fp64 [n, d]
    array or tensor (compared as fp64 against the model's fp64 thresholds)."""
    import torch

    from . import engine

    if isinstance(X, engine.PoolState):
        return engine.forest_regress(model, X.x, X.n, X.d, X.d, X.device, f64=False)
    dev = engine._require_cuda(device)
    x = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(X))
    if x.dim() != 2:
        raise ValueError("X must be a 2-D [rows, features] array")
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError("X must be fp32 or fp64")
    x = x.to(dev).contiguous()
    return engine.forest_regress(model, x, int(x.shape[0]), int(x.shape[1]), int(x.shape[1]), dev,
                                 f64=x.dtype == torch.float64)


# ------------------------------------------------ level steps (sharded fits)
class HipSteps:
    """The local half of a row-sharded fit (dal.parallel.train_classifier /
    train_regressor) on the GPU: the level-step entries of include/dal.h over
    one rank's rows.  Everything is enqueued on the current stream; no method
    reads the device.  Tests replace it with a restatement of the same
    methods (the ``steps`` argument):

      rows(x_local, regress)             the rank's rows as a [n_local, d] tensor
      find_splits(sample, ns, regress)   (thresholds, n_splits, status [1]) of the gathered sample
      begin(job)                         bin the local rows, open the roots
      level_stats(level) -> tensor       the level's totals + histogram of the local rows (integers, 1-D)
      split(level, reduced)              leaf or best split per node from the sums over all ranks
      finish() -> arrays                 (inner, leaf) or (feature, threshold, leaf) of the job's trees

    ``job`` (a SimpleNamespace): regress, x (from rows), y (class-id bytes or
    fp64 labels, numpy), weights int32 [T, n_local], subsets int32 [T, 2^D - 1,
    m], thresholds / n_splits (from find_splits), ns, m, max_depth,
    min_instances, min_gain, num_classes, fmt = (q_y, k_y, q_sq, k_sq), and
    cache, a dict that lives as long as the fit (a regressor's tree chunks
    share their binned rows through it)."""

    def __init__(self, device=None):
        from .engine import _require_cuda

        self.dev = _require_cuda(device)

    def rows(self, x_local, regress: bool):
        return device_rows(x_local, self.dev, keep_f64=regress)

    def find_splits(self, sample, ns: int, regress: bool):
        return device_find_splits(sample, None, ns, f64_thresholds=regress)

    def begin(self, job) -> None:
        import ctypes

        import torch

        lib = _lib.load()
        dev, x, c = self.dev, job.x, job.cache
        n, d = int(x.shape[0]), int(x.shape[1])
        s = _stream(dev)
        if "y" not in c:
            c["y"] = torch.from_numpy(np.ascontiguousarray(job.y)).to(dev)
            if job.regress:
                c["bins"] = torch.empty((n, d), dtype=torch.uint8, device=dev)
                if n:
                    call("dal_rf_bin_rows", x.data_ptr(), _lib.DAL_X_F64 if x.dtype == torch.float64 else
                         _lib.DAL_X_F32, n, d, d, job.thresholds.data_ptr(), job.n_splits.data_ptr(),
                         c["bins"].data_ptr(), s)
        w = torch.from_numpy(np.ascontiguousarray(job.weights, dtype=np.int32)).to(dev)
        sub = torch.from_numpy(np.ascontiguousarray(job.subsets, dtype=np.int32)).to(dev)
        T, n_inner = int(w.shape[0]), (1 << job.max_depth) - 1
        self.blob = ctypes.create_string_buffer(_lib.DAL_RF_JOB_BYTES)
        grow = (job.ns, w.data_ptr(), sub.data_ptr(), job.m, T, job.max_depth, int(job.min_instances),
                float(job.min_gain))
        if job.regress:
            q_y, k_y, q_sq, k_sq = job.fmt
            self.name = "dal_rf_train_regressor"
            wsb = int(lib.dal_rf_train_regressor_workspace_bytes(max(n, 1), T, job.max_depth, job.m, job.ns, k_y,
                                                                 k_sq))
            self.out = (torch.empty((T, n_inner), dtype=torch.int32, device=dev),
                        torch.empty((T, n_inner), dtype=torch.float64, device=dev),
                        torch.empty((T, n_inner + 1), dtype=torch.float64, device=dev))
            self.ws, wsp = _workspace(wsb, dev)
            call(self.name + "_begin", self.blob, c["bins"].data_ptr(), n, d, c["y"].data_ptr(),
                 job.thresholds.data_ptr(), job.n_splits.data_ptr(), *grow, q_y, k_y, q_sq, k_sq,
                 *(o.data_ptr() for o in self.out), wsp, wsb, s)
        else:
            multi = int(job.num_classes) > 2
            self.name = "dal_rf_train_multiclass" if multi else "dal_rf_train"
            wsb = int(lib.dal_rf_train_multiclass_workspace_bytes(max(n, 1), d, T, job.max_depth, job.m, job.ns,
                                                                  int(job.num_classes))) if multi else \
                int(lib.dal_rf_train_workspace_bytes(max(n, 1), d, T, job.max_depth, job.m, job.ns))
            self.out = (torch.empty((T, n_inner, 2), dtype=torch.int32, device=dev),
                        torch.empty((T, n_inner + 1), dtype=torch.uint8, device=dev))
            self.ws, wsp = _workspace(wsb, dev)
            classes = (int(job.num_classes),) if multi else ()
            call(self.name + "_begin", self.blob, x.data_ptr(), n, d, d, c["y"].data_ptr(),
                 job.thresholds.data_ptr(), job.n_splits.data_ptr(), *grow, *classes,
                 *(o.data_ptr() for o in self.out), wsp, wsb, s)
        self.keep = (x, w, sub, job.thresholds, job.n_splits, c)  # what the job points at, for its lifetime

    def level_stats(self, level: int):
        """The span dal_rf_train*_level_span names, as a view of the workspace."""
        import ctypes

        import torch

        call(self.name + "_level_stats", self.blob, int(level), _stream(self.dev))
        ptr, kind, count = ctypes.c_void_p(), ctypes.c_int32(), ctypes.c_int64()
        call(self.name + "_level_span", self.blob, int(level), ctypes.byref(ptr), ctypes.byref(kind),
             ctypes.byref(count))
        dtype, size = (torch.int64, 8) if kind.value == _lib.DAL_RF_SPAN_I64 else (torch.int32, 4)
        off = ptr.value - self.ws.data_ptr()
        self.span = self.ws[off:off + count.value * size].view(dtype)
        return self.span

    def split(self, level: int, reduced) -> None:
        if reduced.data_ptr() != self.span.data_ptr():
            self.span.copy_(reduced)
        call(self.name + "_level_split", self.blob, int(level), _stream(self.dev))

    def finish(self):
        call(self.name + "_finish", self.blob, _stream(self.dev))
        return self.out
