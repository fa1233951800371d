"""LAL query selection -- drop-in for ``ActiveLearnerLAL.selectNext`` of
lal_direct_mllib_implementation/classes/active_learner.py:240-343 ("Learning
Active Learning", Konyushkova, Sznitman, Fua).

The reference feeds five features per unlabeled row to a regression forest
(``self.lalModel.predict``, :319; 2,000 trees, :363) and takes the row with
the largest predicted error reduction:

  f1 = v / T (:280)            f2 = getSD(v, T) (:232-236, :283)
  f3 = positives / nLabeled (:288)
  f6 = mean of f2 over the unlabeled rows (:292)        f8 = nLabeled (:296)

f1 and f2 depend on a row only through its vote count v in {0..T}; f3, f6 and
f8 are per-step scalars.  The regressor's output is therefore a function of v
alone: here it is evaluated on T + 1 rows (not on every unlabeled row) and
indexed by the votes.  f6 needs the histogram of the votes first, so the step
is votes -> histogram -> rows -> regressor -> rescore -> top-k
(dal.engine.lal_step), all on the device.

Canonical arithmetic (fp64, Python-float operation order, no FMA):
  f6 = (((0.0 + float(h[0]) * f2[0]) + float(h[1]) * f2[1]) + ...) / float(nU)
with h the vote histogram of the unlabeled rows -- the reference's per-row sum
in Spark's reduce order depends on the partitioning and pins nothing.
Selection: DESCENDING score, ties to the lower index.  (The reference's
``sortBy(...).max()[0]`` at :328 takes the max over (index, score) tuples and
so returns the largest INDEX; the largest predicted error reduction is what
the method intends.)
"""
from __future__ import annotations

import math

import numpy as np

from .engine import Selection, as_pool_state, lal_step
from .forest import Forest, RegressionForest


def lal_tables(n_trees: int):
    """(f1, f2) fp64 [T + 1]: v / T and getSD(v, T) for v = 0..T, in the
    reference's Python float arithmetic (active_learner.py:280, :232-236).
    Computed on the host once per T; the device never evaluates ** or sqrt."""
    T = int(n_trees)
    if T < 2:
        raise ValueError(f"LAL needs at least 2 trees (getSD divides by T - 1), not {T}")
    f1 = np.empty(T + 1, dtype=np.float64)
    f2 = np.empty(T + 1, dtype=np.float64)
    for v in range(T + 1):
        s = float(v)
        mean = s / T
        f1[v] = s / T
        f2[v] = math.sqrt((s * ((1 - mean) ** 2) + (T - s) * (mean ** 2)) / (T - 1))
    return f1, f2


def select_lal(pool, unlabeled_idx, forest: Forest, lal_model: RegressionForest, k: int, n_labeled: int,
               n_positive: int, device=None) -> Selection:
    """Score every unlabeled row with the LAL regressor and select the k with
    the largest predicted error reduction.

    pool           [N, D] fp32 (numpy or torch; or a PoolState to reuse caches)
    unlabeled_idx  global row indices of the unlabeled set (not empty)
    forest         binary dal.forest.Forest of T >= 2 trees (the classifier)
    lal_model      dal.forest.RegressionForest over the five LAL features
    k              batch size (clamped to the unlabeled count)
    n_labeled      size of the labeled set (>= 1); n_positive: the sum of its
                   0/1 labels
    Returns Selection(scores[U], indices[k], selected_scores[k], votes[U])
    with the attribute ``lut`` (fp64 [T + 1] on the device): the regressor's
    prediction per vote count, scores[i] = lut[votes[i]].
    """
    if not isinstance(lal_model, RegressionForest):
        raise TypeError("lal_model must be a dal.forest.RegressionForest")
    state = as_pool_state(pool, device=device)
    return lal_step(state, unlabeled_idx, forest, lal_model, k, n_labeled, n_positive)


LAL_FEATURE_COLUMNS = (0, 1, 2, 5, 7)  # active_learner.py:356; the label is the last column


def lal_training_set(table):
    """(X fp64 [n, 5], y fp64 [n]) from the LAL regression table
    (active_learner.py:354-356): an [n, >= 9] array, or the path of a text
    file of whitespace-separated numbers, one row per line.  Features are
    columns 0, 1, 2, 5, 7 and the label is the last column."""
    is_path = isinstance(table, (str, bytes)) or hasattr(table, "__fspath__")
    t = np.loadtxt(table, dtype=np.float64, ndmin=2) if is_path else np.asarray(table, dtype=np.float64)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 9:
        raise ValueError("the LAL table must be a non-empty [n, >= 9] array")
    return np.ascontiguousarray(t[:, list(LAL_FEATURE_COLUMNS)]), np.ascontiguousarray(t[:, -1])


def train_lal_model(table, num_trees: int = 2000, **kwargs) -> RegressionForest:
    """The LAL regressor of active_learner.py:354-363,
    ``RandomForest.trainRegressor(reg, numTrees=2000, categoricalFeaturesInfo={})``,
    trained on the GPU (dal.random_forest.train_regressor; ``kwargs`` are its
    keyword arguments).  The result is what ``select_lal`` and
    ``run_loop(strategy="lal", lal_model=...)`` take."""
    from .random_forest import train_regressor

    X, y = lal_training_set(table)
    return train_regressor(X, y, num_trees=num_trees, **kwargs)


__all__ = ["lal_tables", "select_lal", "train_lal_model", "lal_training_set", "Selection", "RegressionForest"]
