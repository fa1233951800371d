"""Test-set evaluation on the GPU: confusion counts, exact ROC AUC, exact MSE.

Reference:
  lal_direct_mllib_implementation/classes/active_learner.py:95-121
      ActiveLearner.evaluate: 'accuracy', 'TN', 'TP', 'FN', 'FP', 'auc' on the
      test split
  final_thesis/uncertainty_sampling.py:80-82, :113   the loops' test accuracy
  mllib/mllib_random_forest_regressor.py:48 (and save_regression_model.py:51,
  mllib_randomforest_regression_lal_randomtree_dataset.py:48)
      testMSE = sum (label - prediction)^2 / count

Every classification measure is a function of one small integer table, the
joint histogram of (vote count, label), which csrc/forest_eval.hip fills in one
fused forest pass that stores nothing per row (dal_forest_evaluate).  The
finish here runs in Python integers: each figure is one ``int / int`` true
division, the correct rounding of an exact rational, so a result is the same
bytes for every row order, grid, chunking and shard count.  The MSE has the
same guarantee from the integer-limb sums of csrc/rf_exact_sum.hpp
(csrc/sq_error.hip).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import DAL_FLAG_NONFINITE, DAL_LAL_MAX_TREES, DAL_MC_MAX_CLASSES, DAL_MC_MAX_TREES, DAL_RF_REG_MAX_LIMBS, call

LIMB_BITS = 31  # csrc/rf_exact_sum.hpp
MAX_ROWS = (1 << 31) - 1
BINARY_MEASURES = ("accuracy", "TN", "FP", "FN", "TP", "auc", "confusion")
MULTICLASS_MEASURES = ("accuracy", "confusion")
_NO_LOW, _NO_TOP = np.iinfo(np.int32).max, np.iinfo(np.int32).min


def table_shape(n_trees: int, n_classes: int):
    """Shape of the joint table (dal_forest_evaluate): (T + 1, 2) for two
    classes, cell [v][y]; (C, C) above, cell [y][pred].  ValueError outside
    the kernels' limits."""
    T, C = int(n_trees), int(n_classes)
    if C == 2:
        if not 1 <= T <= DAL_LAL_MAX_TREES:
            raise ValueError(f"a two-class forest is evaluated with 1..{DAL_LAL_MAX_TREES} trees, not {T}")
        return T + 1, 2
    if not 3 <= C <= DAL_MC_MAX_CLASSES:
        raise ValueError(f"n_classes must lie in [2, {DAL_MC_MAX_CLASSES}], not {C}")
    if not 1 <= T <= DAL_MC_MAX_TREES:
        raise ValueError(f"a forest of {C} classes is evaluated with 1..{DAL_MC_MAX_TREES} trees, not {T}")
    return C, C


def check_measures(measures, n_classes: int):
    """The measure names as a tuple, or ValueError: an unknown name, or a
    binary measure ('auc', 'TN', ...) asked of a forest of more than two
    classes."""
    names = (measures,) if isinstance(measures, str) else tuple(measures)
    for m in names:
        if m not in BINARY_MEASURES:
            raise ValueError(f"unknown measure {m!r} (known: {', '.join(BINARY_MEASURES)})")
        if int(n_classes) > 2 and m not in MULTICLASS_MEASURES:
            raise ValueError(f"measure {m!r} is defined for two classes, not for n_classes = {int(n_classes)}")
    return names


def check_labels(y, n: int, forest) -> np.ndarray:
    """The test labels as n class-id bytes, or ValueError.  A forest that
    carries labels (``classes_``) maps them to ids; otherwise y holds the ids.
    The kernel counts a label >= n_classes nowhere, so it is refused here."""
    yv = np.asarray(y).reshape(-1)
    if yv.shape[0] != n:
        raise ValueError(f"y_test must hold {n} labels, one per row")
    C = int(forest.n_classes)
    if forest.classes_ is not None:
        classes = np.asarray(forest.classes_)
        ids = np.searchsorted(classes, yv)
        ok = (ids < classes.size) & (classes[np.minimum(ids, classes.size - 1)] == yv)
        if not ok.all():
            raise ValueError("y_test holds a label the forest's classes_ do not")
        yv = ids
    if yv.size and not np.isin(yv, np.arange(C)).all():
        raise ValueError(f"test labels must be class ids in [0, {C})")
    return np.ascontiguousarray(yv.astype(np.uint8))


def finish(table, n_trees: int, n_classes: int, measures=("accuracy",)) -> dict:
    """The measures from the joint table, in Python integers (pure host code).

    Two classes, table [T + 1][2] = H[v][y] (the prediction is ``2 v > T``,
    dal.random_forest.predict's rule: ties go to class 0):
      'TN', 'FP', 'FN', 'TP'  the cells of the reference's
                  confusion_matrix[true][pred], Python ints
      'accuracy'  (TP + TN) / n, a fraction as in accuracy_score; NaN for n == 0
      'auc'       sum_v H[v][1] (2 sum_{u<v} H[u][0] + H[v][0]) / (2 P N): the
                  exact area under the ROC of the score v / T, ties counted
                  half; NaN when P N == 0.  The score is the HARD-VOTE fraction
                  the distributed code uses (active_learner.py:280), not
                  scikit-learn's averaged leaf probability.
      'confusion' int64 [2][2]
    More classes, table [C][C] = H[y][pred]: 'accuracy' (the trace over n) and
    'confusion' (int64 [C][C])."""
    T, C = int(n_trees), int(n_classes)
    names = check_measures(measures, C)
    shape = table_shape(T, C)
    H = [[int(c) for c in row] for row in np.asarray(table).reshape(shape)]
    out = {}
    if C > 2:
        n = sum(sum(r) for r in H)
        for m in names:
            if m == "accuracy":
                out[m] = sum(H[c][c] for c in range(C)) / n if n else float("nan")
            else:
                out[m] = np.array(H, dtype=np.int64)
        return out
    tn = sum(H[v][0] for v in range(T + 1) if 2 * v <= T)
    fp = sum(H[v][0] for v in range(T + 1) if 2 * v > T)
    fn = sum(H[v][1] for v in range(T + 1) if 2 * v <= T)
    tp = sum(H[v][1] for v in range(T + 1) if 2 * v > T)
    neg, pos = tn + fp, fn + tp
    for m in names:
        if m == "accuracy":
            out[m] = (tp + tn) / (neg + pos) if neg + pos else float("nan")
        elif m == "auc":
            below, num = 0, 0
            for v in range(T + 1):
                num += H[v][1] * (2 * below + H[v][0])
                below += H[v][0]
            out[m] = num / (2 * pos * neg) if pos * neg else float("nan")
        elif m == "confusion":
            out[m] = np.array([[tn, fp], [fn, tp]], dtype=np.int64)
        else:
            out[m] = {"TN": tn, "FP": fp, "FN": fn, "TP": tp}[m]
    return out


def joint_histogram(forest, state, labels_dev, flags=None, build_blocked: bool = True):
    """The joint table of ``forest`` over the rows of ``state`` (a PoolState)
    as a device int64 tensor of table_shape: one dal_forest_evaluate call,
    stream-ordered, no per-row output.  labels_dev: uint8 [n] class ids on the
    device (check_labels); flags: uint8 [n] device row flags, the rows carrying
    DAL_ROW_CANDIDATE are counted (None: all).  The blocked kernel runs over
    the pool's blocked copy with the prepared forest where
    dal_forest_evaluate_blocked_rows allows (``build_blocked``: build the copy
    when the pool has none yet), else the row-major kernel."""
    import torch

    from .engine import _ptr, _stream

    lib = _lib.load()
    T, C = forest.n_trees, int(forest.n_classes)
    shape = table_shape(T, C)
    forest.check_features(state.d)
    forest.check_classes()
    dev = state.device
    if labels_dev.dtype != torch.uint8 or labels_dev.numel() != state.n:
        raise ValueError(f"labels must be {state.n} uint8 class ids on the device")
    if flags is not None and (flags.dtype != torch.uint8 or flags.numel() != state.n):
        raise ValueError(f"flags must be {state.n} uint8 row flags on the device")
    inner, leaf = forest.device(dev)
    xb = prep = None
    if lib.dal_forest_evaluate_blocked_rows(state.d, T, forest.depth, C):
        xb = state.blocked_pool(forest, build=build_blocked, multiclass=C > 2)
        prep = None if xb is None else forest.blocked_prep(dev, state.d)
        if prep is None:
            xb = None
    hist = torch.zeros(shape, dtype=torch.int64, device=dev)
    if state.n == 0:  # (an empty shard: nothing to launch)
        return hist
    call("dal_forest_evaluate", _ptr(state.x), 0 if xb is None else _ptr(xb), 0 if prep is None else _ptr(prep),
         state.n, state.d, state.d, _ptr(inner), _ptr(leaf), T, forest.depth, C, _ptr(labels_dev),
         0 if flags is None else _ptr(flags), _ptr(hist), _stream(dev))
    return hist


def evaluate(forest, X_test, y_test, measures=("accuracy",), flags=None, device=None, hist_fn=None) -> dict:
    """ActiveLearner.evaluate on the GPU: the measures of ``finish`` for
    ``forest`` (a dal.forest.Forest) on the test split.  X_test: an [n, d]
    array or a PoolState (which reuses its blocked copy and the prepared
    forest); y_test: n labels (class ids, or the forest's ``classes_`` labels),
    uploaded as uint8; flags: optional uint8 [n] row flags, only rows carrying
    DAL_ROW_CANDIDATE are evaluated.  hist_fn(x, y_ids, forest) -> table
    replaces the HIP kernel (tests inject the restatement; None: the kernel).
    'auc' scores a row by its hard-vote fraction v / T (active_learner.py:280),
    not by scikit-learn's averaged leaf probability."""
    names = check_measures(measures, forest.n_classes)
    T, C = forest.n_trees, int(forest.n_classes)
    table_shape(T, C)
    if hist_fn is not None:
        x = np.asarray(X_test)
        y = check_labels(y_test, x.shape[0], forest)
        if flags is not None:
            keep = (np.asarray(flags).reshape(-1) & _lib.DAL_ROW_CANDIDATE) != 0
            x, y = x[keep], y[keep]
        table = hist_fn(x, y, forest)
        return finish(np.asarray(table), T, C, names)
    import torch

    from .engine import PoolState

    pooled = isinstance(X_test, PoolState)
    state = X_test if pooled else PoolState(X_test, device=device)
    labels_dev = torch.from_numpy(check_labels(y_test, state.n, forest)).to(state.device)
    if flags is not None:
        if not isinstance(flags, torch.Tensor):
            flags = torch.from_numpy(np.ascontiguousarray(flags, dtype=np.uint8))
        flags = flags.to(device=state.device, dtype=torch.uint8).contiguous()
    hist = joint_histogram(forest, state, labels_dev, flags, build_blocked=pooled)
    return finish(hist.cpu().numpy(), T, C, names)


# ------------------------------------------------------------------- MSE --
def sq_error_limbs(low: int, top: int):
    """(q, k) of the exact sum from the format pass's (low, top), as
    dal.random_forest.exact_sum_format derives them: q = low, k = max(1,
    ceil((top - low) / 31)); (0, 1) when every square is zero.  ValueError
    naming the span when it needs more than DAL_RF_REG_MAX_LIMBS limbs."""
    low, top = int(low), int(top)
    if low == _NO_LOW or top == _NO_TOP:
        return 0, 1
    span = top - low
    k = max(1, -(-span // LIMB_BITS))
    if k > DAL_RF_REG_MAX_LIMBS:
        raise ValueError(f"the squared errors span {span} bits between their highest and lowest set bit, more than "
                         f"the {DAL_RF_REG_MAX_LIMBS * LIMB_BITS} the exact sum holds")
    return low, k


def mse_from_cells(words, q: int, n: int) -> float:
    """MSE = (2^q sum_j word_j 2^(31 j)) / n: one rounding of the exact
    rational (2^q folded into the numerator or the denominator as integers);
    NaN for n == 0."""
    n = int(n)
    if n == 0:
        return float("nan")
    total = sum(int(w) << (LIMB_BITS * j) for j, w in enumerate(np.asarray(words).reshape(-1)))
    q = int(q)
    return (total << q) / n if q >= 0 else total / (n << -q)


def sq_error_cells(pred, y):
    """The exact sum of fl(fl(y - pred)^2) over two fp64 device vectors:
    (words int64 numpy [k], q).  dal_sq_error_format, the host's (q, k), then
    dal_sq_error_accumulate.  ValueError for a non-finite square or a span
    past the limb limit."""
    import torch

    from .engine import _ptr, _stream

    n = int(pred.numel())
    if int(y.numel()) != n or pred.dtype != torch.float64 or y.dtype != torch.float64:
        raise ValueError("pred and y must be fp64 vectors of one length")
    if n > MAX_ROWS:
        raise ValueError(f"{n} rows: the exact sum takes at most {MAX_ROWS}")
    if n == 0:
        return np.zeros(1, dtype=np.int64), 0
    dev = pred.device
    fmt = torch.tensor([_NO_LOW, _NO_TOP, 0], dtype=torch.int32, device=dev)
    s = _stream(dev)
    base, step = fmt.data_ptr(), fmt.element_size()
    call("dal_sq_error_format", _ptr(pred), _ptr(y), n, base, base + step, base + 2 * step, s)
    low, top, status = (int(v) for v in fmt.cpu().numpy())
    if status & DAL_FLAG_NONFINITE:
        raise ValueError("a squared error is not finite (a NaN or infinite label or prediction, or an overflow)")
    q, k = sq_error_limbs(low, top)
    cells = torch.zeros(k, dtype=torch.int64, device=dev)
    call("dal_sq_error_accumulate", _ptr(pred), _ptr(y), n, q, k, _ptr(cells), s)
    return cells.cpu().numpy(), q


def mean_squared_error(model, X, y, device=None) -> float:
    """testMSE of a regression forest (mllib_random_forest_regressor.py:48):
    sum_i fl(fl(y_i - pred_i)^2) / n with pred = dal_forest_regress's fp64
    prediction, the sum exact and the quotient rounded once: the same bits
    for every row order and chunking.  model: a dal.forest.RegressionForest;
    X: a PoolState or an fp32 / fp64 [n, d] array or tensor; y: n real labels."""
    import torch

    from .random_forest import predict_regression

    pred = predict_regression(model, X, device=device)
    yv = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
    yv = np.ascontiguousarray(yv.reshape(-1), dtype=np.float64)
    if yv.shape[0] != int(pred.numel()):
        raise ValueError(f"y must hold {int(pred.numel())} labels, one per row")
    words, q = sq_error_cells(pred, torch.from_numpy(yv).to(pred.device))
    return mse_from_cells(words, q, yv.shape[0])
