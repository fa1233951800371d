"""Test-side restatement of dal.metrics (not a test): the joint table by a
per-row Python loop over the oracle's / multiclass_reference's votes, the
measures as fractions.Fraction, the MSE as float(sum(Fraction(s_i)) / n).

Two classes: table[v][y], v = the number of trees voting 1; the prediction is
2 v > T (ties to class 0).  More classes: table[y][pred], pred the lowest
class with the most trees.  A row with a label >= C, or with a tree whose leaf
byte is >= C, is counted nowhere.
"""
from fractions import Fraction

import numpy as np

import multiclass_reference as MR
from oracle import dal_oracle as O


def leaf_classes(forest, X):
    """[T, n] leaf value of every tree for every row: a dal.forest.Forest
    (heap arrays) or an oracle.OracleForest."""
    if isinstance(forest, O.OracleForest):
        return O.tree_predictions(forest, X).astype(np.int64)
    return MR.tree_leaves(forest.inner, forest.leaf, forest.depth, X)


def joint_table(forest, X, y, n_classes=None, flags=None):
    """The joint table as nested lists of Python ints."""
    C = int(forest.n_classes if n_classes is None else n_classes)
    lv = leaf_classes(forest, X)
    T, n = lv.shape
    table = [[0] * 2 for _ in range(T + 1)] if C == 2 else [[0] * C for _ in range(C)]
    for i in range(n):
        if flags is not None and not (int(flags[i]) & 1):
            continue
        yi = int(y[i])
        col = [int(c) for c in lv[:, i]]
        if yi >= C or any(c >= C for c in col):
            continue
        if C == 2:
            table[sum(1 for c in col if c == 1)][yi] += 1
        else:
            cnt = [col.count(c) for c in range(C)]
            table[yi][cnt.index(max(cnt))] += 1
    return table


def _ratio(num, den):
    return float(Fraction(num, den)) if den else float("nan")


def measures(table, n_trees, n_classes, names):
    """The dict of dal.metrics.finish from fractions."""
    T, C = int(n_trees), int(n_classes)
    H = [[int(c) for c in row] for row in table]
    out = {}
    if C > 2:
        n = sum(sum(r) for r in H)
        for m in names:
            out[m] = _ratio(sum(H[c][c] for c in range(C)), n) if m == "accuracy" else np.array(H, dtype=np.int64)
        return out
    cm = [[0, 0], [0, 0]]
    for v in range(T + 1):
        for yy in (0, 1):
            cm[yy][1 if 2 * v > T else 0] += H[v][yy]
    (tn, fp), (fn, tp) = cm
    neg, pos = tn + fp, fn + tp
    for m in names:
        if m == "accuracy":
            out[m] = _ratio(tp + tn, neg + pos)
        elif m == "auc":
            # P(score of a positive > score of a negative) + P(equal) / 2
            wins = Fraction(0)
            for v in range(T + 1):
                wins += H[v][1] * (sum(H[u][0] for u in range(v)) + Fraction(H[v][0], 2))
            out[m] = float(wins / (pos * neg)) if pos * neg else float("nan")
        elif m == "confusion":
            out[m] = np.array(cm, dtype=np.int64)
        else:
            out[m] = {"TN": tn, "FP": fp, "FN": fn, "TP": tp}[m]
    return out


def evaluate(forest, X, y, names, flags=None):
    return measures(joint_table(forest, X, y, flags=flags), forest.n_trees, forest.n_classes, names)


def hist_fn(x, y, forest):
    """The local step dal.metrics.evaluate / dal.parallel.evaluate inject."""
    import torch

    x = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    y = y.numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
    return torch.tensor(joint_table(forest, x, y), dtype=torch.int64)


def same(a, b):
    """Two measure dicts hold the same keys and the same bytes."""
    if list(a) != list(b):
        return False
    for k in a:
        va, vb = a[k], b[k]
        if isinstance(va, np.ndarray) or isinstance(vb, np.ndarray):
            if not (isinstance(va, np.ndarray) and isinstance(vb, np.ndarray) and va.dtype == vb.dtype
                    and va.shape == vb.shape and va.tobytes() == vb.tobytes()):
                return False
        elif isinstance(va, float) or isinstance(vb, float):
            if not (isinstance(va, float) and isinstance(vb, float)
                    and np.float64(va).tobytes() == np.float64(vb).tobytes()):
                return False
        elif type(va) is not type(vb) or va != vb:
            return False
    return True


def squared_errors(pred, y):
    """s_i = fl(fl(y_i - pred_i)^2) as fp64 (numpy: one rounding per operation)."""
    e = np.asarray(y, dtype=np.float64) - np.asarray(pred, dtype=np.float64)
    with np.errstate(over="ignore"):
        return e * e


def mse(pred, y):
    s = squared_errors(pred, y)
    if s.size == 0:
        return float("nan")
    return float(sum((Fraction(float(v)) for v in s), Fraction(0)) / s.size)


def sum_format(s):
    """(low, top) over the nonzero values in Python integers: the exponent of
    the lowest set bit and the exponent above the highest set bit; None when
    every value is zero."""
    low = top = None
    for v in s:
        fr = Fraction(float(v))
        if fr == 0:
            continue
        num, den = abs(fr.numerator), fr.denominator  # den a power of two
        tz = (num & -num).bit_length() - 1
        lo = tz - (den.bit_length() - 1)
        hi = num.bit_length() - (den.bit_length() - 1)
        low = lo if low is None else min(low, lo)
        top = hi if top is None else max(top, hi)
    return low, top
