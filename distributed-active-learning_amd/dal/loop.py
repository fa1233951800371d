"""Active-learning loop driver and pool ingest.

Reproduces the end-to-end behaviour of the reference scripts around the
GPU query step:

  ingest     uncertainty_sampling.py:37-42 / density_weighting.py:45-53,59-65:
             whitespace text, label in the last column, -1 -> 0, optional
             take(n_samples) truncation
  loop       uncertainty_sampling.py:59-114, density_weighting.py:106-179,
             random_sampling.py:60-94: labeled = range(window_size) at start;
             each iteration trains a forest on the labeled rows, measures test
             accuracy, selects window_size rows and moves them to the labeled set;
             stops when the unlabeled set is empty
  log        ``labeled =  L  unlabeled =  U`` (:65) and
             ``Iteration  i  -- accu =  a`` (:113)

Forest training (RandomForest.trainClassifier, uncertainty_sampling.py:71-76)
runs on the GPU by default (dal.random_forest: MLlib 2.1's gini / maxDepth 4 /
maxBins 32 / sqrt-feature algorithm, seeded bagging draws; binary labels, or
C classes when ``num_classes`` is given); trainer="sklearn"
keeps the scikit-learn fit of round 1.  The selection step is the GPU path
(dal.uncertainty_sampling / dal.density_weighting).  The random baseline
(random_sampling.py:88-89, ``sortBy(np.random.uniform).take``) has no
arithmetic and runs on the host.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np


def load_labeled_text(path: str, n_samples=None, label_map: str = "reference"):
    """Whitespace-separated rows, features then label.  label_map="reference"
    applies the scripts' ``0 if int(label) == -1 else 1`` (uncertainty_sampling.py:39,
    written for the +-1 striatum labels); "as_is" keeps 0/1 labels (the LAL
    checkerboard files).  Returns (X fp32 [N, D], y int64 [N]).  Parsed by the
    native multi-threaded parser (dal.ingest; dal.ingest.load_pool uploads the
    pool to HBM through pinned memory instead)."""
    from .ingest import parse_labeled_text

    return parse_labeled_text(path, n_samples=n_samples, label_map=label_map)


class GpuForestModel:
    """A forest trained by dal.random_forest, with MLlib's RandomForestModel
    ``predict`` (majority vote) on the GPU."""

    def __init__(self, forest, device=None):
        self.forest = forest
        self.device = device

    def predict(self, X):
        """Labels: ``forest.classes_[class id]`` where the forest carries labels."""
        from .random_forest import predict

        labels, _ = predict(self.forest, X, device=self.device)
        labels = labels.cpu().numpy()
        return labels if self.forest.classes_ is None else np.asarray(self.forest.classes_)[labels]


def train_forest(X, y, n_estimators: int = 10, seed: int = 0, max_depth: int = 4, trainer="gpu",
                 device=None, num_classes=None):
    """RandomForest.trainClassifier(numTrees=T, featureSubsetStrategy='auto',
    impurity='gini') with MLlib's default maxDepth=4.  trainer: "gpu"
    (dal.random_forest), "sklearn", or a callable (X, y, T, seed) -> model with
    ``predict``.  num_classes: MLlib's numClasses for the GPU trainer (y then
    holds class ids in [0, num_classes)); None = binary labels in {0, 1}."""
    if callable(trainer):
        return trainer(X, y, n_estimators, seed)
    if trainer == "gpu":
        from .random_forest import train_classifier

        kw = {} if num_classes is None else {"num_classes": int(num_classes)}
        return GpuForestModel(train_classifier(X, y, n_estimators, max_depth=max_depth, seed=seed,
                                               device=device, **kw), device)
    if trainer != "sklearn":
        raise ValueError(f"unknown trainer {trainer!r}")
    from sklearn.ensemble import RandomForestClassifier

    rf = RandomForestClassifier(n_estimators=n_estimators, max_depth=max_depth,
                                max_features="sqrt", bootstrap=True, random_state=seed)
    rf.fit(X, y)
    return rf


@dataclass
class LoopResult:
    labeled_history: list = field(default_factory=list)  # selected indices per iteration
    accuracy: list = field(default_factory=list)  # test accuracy (%) per iteration
    log: list = field(default_factory=list)
    metrics: list = field(default_factory=list)  # dal.metrics.evaluate's dict per iteration (run_loop(measures=))


# the strategies that score with the density (``density_over`` applies; E starts as the initial labeled rows)
DENSITY_STRATEGIES = ("density", "information_density", "soft_information_density")


def run_loop(X, y, X_test=None, y_test=None, strategy: str = "uncertainty",
             window_size: int = 10, n_estimators: int = 10, max_iterations=None,
             seed: int = 0, select_fn=None, device=None, beta: float = 1.0,
             verbose: bool = False, trainer="gpu", num_classes=None, lal_model=None,
             initial_labeled=None, measures=None, hist_fn=None, density_over: str = "initial",
             alpha=None, sim_pool=None, soft_votes: bool = False) -> LoopResult:
    """Run the AL loop.  strategy: "uncertainty" (uncertainty_sampling.py),
    "density" (density_weighting.py, E = L0 = range(window_size)),
    "information_density" (class entropy x density, E = L0;
    density_weighting.select_multiclass), "soft_information_density"
    (entropy(predict_proba) x density over the averaged leaf class
    distributions, E = L0; density_weighting.select_soft: soft votes, below,
    for any label count), "bald" (the trees' disagreement H(pbar) - mean_t
    H(p_t) over the leaf class distributions, the mean KL divergence to the
    consensus: dal.uncertainty_sampling.select(strategy="bald"); soft votes,
    below, for any label count), "lal" (ActiveLearnerLAL.selectNext,
    lal_direct_mllib_implementation/classes/active_learner.py:240-343:
    dal.active_learner.select_lal with ``lal_model``, a
    dal.forest.RegressionForest over the five LAL features; binary only; the
    labeled count and its positives come from the current labeled set),
    "ranked_batch" (dal.uncertainty_sampling.select_batch: the least-confidence
    weight x diversity greedy batch against the current labeled set; binary or
    ``num_classes``; ``alpha`` and ``sim_pool`` are passed on and belong to
    this strategy alone) or "random".
    trainer: see train_forest.  Labels of more than two values: "uncertainty"
    and "information_density" score the C-class forest
    (Forest.from_sklearn(rf, multiclass=True)) and need trainer="sklearn" or a
    callable, or trainer="gpu" with ``num_classes`` (below); "density" is
    binary, as is trainer="gpu" without ``num_classes``: both raise ValueError.
    num_classes: MLlib's numClasses, at least the number of distinct values
    of y (explicit, because a labeled window can lack a class).  The GPU
    trainer then fits C-class forests on the class ids (the position of a label
    in np.unique(y)) and the forest's ``classes_`` maps ids back to labels;
    train -> score -> select then all run on the GPU.
    "information_density" takes the per-class votes for any label count (two
    labels: the two-term entropy, from any trainer).

    ``select_fn(strategy, pool, unlabeled, model, k) -> indices`` can replace
    the GPU step (tests use the oracle); by default the dal GPU path runs.

    initial_labeled: the rows the loop starts from, in that order (distinct
    indices in [0, n); dal.dataset.Dataset.set_start_state gives the LAL
    classes' start); ``unlabeled`` is the ascending remainder and, for the
    density strategies, E is that set.  None: labeled = range(window_size).

    measures: a tuple of dal.metrics measure names ('accuracy', 'TN', 'FP',
    'FN', 'TP', 'auc', 'confusion').  With a test split every iteration then
    appends dal.metrics.evaluate's dict for the iteration's forest to
    ``LoopResult.metrics`` (ActiveLearner.evaluate, active_learner.py:95-121):
    one dal_forest_evaluate call on the test pool, uploaded once with its
    labels; a scikit-learn model goes through Forest.from_sklearn.  hist_fn:
    dal.metrics.evaluate's (tests inject the restatement; None: the HIP
    kernel).  measures=None changes nothing: same calls, log and ``accuracy``.

    density_over ("density", "information_density" and
    "soft_information_density" only): which rows the
    density d_i = sum_{j not in E} cos(x_i, x_j) sums over.  "initial" (the
    default) is the reference: E is frozen at the rows the loop starts from,
    so every row labeled later keeps contributing to every density
    (density_weighting.py:95-100 drops L0 once, before the loop).
    "unlabeled" DEPARTS from the reference: E is the current labeled set, the
    usual definition of information density (an average similarity to the
    pool still to be queried).  After each selection the loop calls
    ``state.exclude(chosen)``, which lowers the cached density by the chosen
    rows' cosine sums (an N x k product) instead of recomputing the N^2 Gram
    -- the cost that made the reference keep E fixed.  With ``select_fn`` the
    value is only validated: the callback sees ``unlabeled`` and can derive E.
    Any other value, or "unlabeled" with a strategy that has no density,
    raises ValueError.

    soft_votes ("uncertainty" and "ranked_batch" only, with trainer="sklearn"
    or a callable that returns a scikit-learn forest): score the averaged leaf
    class distributions (scikit-learn's ``predict_proba``; modAL's uncertainty
    sampling) instead of the hard votes -- every iteration's forest goes
    through dal.forest.ProbabilityForest.from_sklearn, for any label count.
    trainer="gpu" (its forests keep no leaf distributions) or any other
    strategy raises ValueError.  False, the default, makes the calls it made.
    strategy="soft_information_density" scores soft votes by definition: it
    needs the same trainers, raises the same error for trainer="gpu", and
    accepts soft_votes=True as redundant.  So does strategy="bald".
    """
    soft_density = strategy == "soft_information_density"  # (soft votes by its definition: the flag is redundant)
    bald = strategy == "bald"  # (likewise)
    if soft_votes or soft_density or bald:
        if not (soft_density or bald) and strategy not in ("uncertainty", "ranked_batch"):
            raise ValueError(f"soft_votes=True belongs to strategy 'uncertainty' or 'ranked_batch': {strategy!r} "
                             "scores hard votes")
        if trainer == "gpu":
            raise ValueError("soft_votes=True needs trainer='sklearn' or a callable returning a scikit-learn "
                             "forest: trainer='gpu' keeps no leaf distributions")
    if density_over not in ("initial", "unlabeled"):
        raise ValueError(f"density_over must be 'initial' or 'unlabeled', not {density_over!r}")
    if density_over == "unlabeled" and strategy not in DENSITY_STRATEGIES:
        raise ValueError(f"density_over='unlabeled' needs strategy 'density', 'information_density' or "
                         f"'soft_information_density': {strategy!r} has no density")
    from .forest import Forest

    # more than two label values: multiclass uncertainty sampling (per-class
    # votes, dal.engine.multiclass_step) over a scikit-learn or caller-trained
    # forest, or one the GPU trainer fits when num_classes is given; density
    # weighting is binary
    if strategy != "ranked_batch" and (alpha is not None or sim_pool is not None):
        raise ValueError("alpha and sim_pool belong to strategy='ranked_batch'")
    classes = np.unique(np.asarray(y))
    multiclass = classes.size > 2
    if num_classes is not None and int(num_classes) < max(classes.size, 2):
        raise ValueError(f"num_classes={num_classes} is less than the {max(classes.size, 2)} label values "
                         "(at least two) it must cover")
    if (multiclass or (num_classes is not None and int(num_classes) > 2)) and strategy == "density":
        raise ValueError("strategy='density' is binary only: y holds more than two label values "
                         "(use strategy='uncertainty')")
    if strategy == "lal":
        if multiclass or (num_classes is not None and int(num_classes) > 2):
            raise ValueError("strategy='lal' is binary only: y holds more than two label values")
        if lal_model is None and select_fn is None:
            raise ValueError("strategy='lal' needs lal_model= (a dal.forest.RegressionForest)")
    if multiclass and trainer == "gpu" and num_classes is None:
        raise ValueError("trainer='gpu' (dal.random_forest) trains binary forests only unless num_classes= is "
                         "given: y holds more than two label values (pass num_classes=, or use "
                         "trainer='sklearn' or a callable)")
    # class ids for the GPU trainer: the label's position in np.unique(y)
    y_fit = np.searchsorted(classes, np.asarray(y)) if num_classes is not None and trainer == "gpu" else y
    n = X.shape[0]
    if initial_labeled is None:
        labeled = list(range(min(window_size, n)))
        unlabeled = np.arange(len(labeled), n, dtype=np.int64)
    else:
        start = np.asarray(initial_labeled, dtype=np.int64).reshape(-1)
        if start.size == 0 or start.min() < 0 or start.max() >= n or np.unique(start).size != start.size:
            raise ValueError("initial_labeled must hold distinct row indices in [0, n)")
        labeled = [int(i) for i in start]
        unlabeled = np.setdiff1d(np.arange(n, dtype=np.int64), start, assume_unique=True)
    res = LoopResult()
    rng = np.random.default_rng(seed)
    state = test_state = test_labels = None
    if select_fn is None and strategy != "random":
        from .engine import PoolState

        excluded = np.asarray(labeled, dtype=np.int64) if strategy in DENSITY_STRATEGIES else None
        state = PoolState(X, excluded=excluded, device=device)
        if sim_pool is not None:
            from .similarity import _bf16_pool

            sim_pool, _ = _bf16_pool(sim_pool, state.device)  # uploaded and rounded once
    it = 1
    while True:
        line = f"labeled =  {len(labeled)}  unlabeled =  {unlabeled.size}"
        res.log.append(line)
        if verbose:
            print(line)
        if unlabeled.size == 0:
            break
        if max_iterations is not None and it > max_iterations:
            break
        lab = np.asarray(labeled)
        rf = train_forest(X[lab], y_fit[lab], n_estimators, seed + it, trainer=trainer, device=device,
                          num_classes=num_classes)
        if y_fit is not y:
            rf.forest.classes_ = classes
        acc = None
        if X_test is not None:
            if isinstance(rf, GpuForestModel) and test_state is None:
                from .engine import PoolState

                test_state = PoolState(X_test, device=device)  # uploaded once
            pred = rf.predict(test_state if isinstance(rf, GpuForestModel) else X_test)
            acc = (1 - np.mean(pred != y_test)) * 100
            if measures is not None:
                from . import metrics

                ev_forest = rf.forest if isinstance(rf, GpuForestModel) else rf if isinstance(rf, Forest) else \
                    Forest.from_sklearn(rf, multiclass=True) if multiclass else Forest.from_sklearn(rf)
                if hist_fn is not None:
                    res.metrics.append(metrics.evaluate(ev_forest, X_test, y_test, measures, hist_fn=hist_fn))
                else:
                    if test_state is None:
                        from .engine import PoolState

                        test_state = PoolState(X_test, device=device)  # uploaded once
                    if test_labels is None:  # uploaded once (the forest's classes_ do not change)
                        import torch

                        test_labels = torch.from_numpy(
                            metrics.check_labels(y_test, test_state.n, ev_forest)).to(test_state.device)
                    names = metrics.check_measures(measures, ev_forest.n_classes)
                    hist = metrics.joint_histogram(ev_forest, test_state, test_labels)
                    res.metrics.append(metrics.finish(hist.cpu().numpy(), ev_forest.n_trees, ev_forest.n_classes,
                                                      names))
        k = min(window_size, unlabeled.size)
        if strategy == "random":
            order = np.argsort(rng.uniform(size=unlabeled.size), kind="stable")
            chosen = unlabeled[order[:k]]
        elif select_fn is not None:
            chosen = np.asarray(select_fn(strategy, X, unlabeled, rf, k))
        else:
            if soft_votes or soft_density or bald:
                from .forest import ProbabilityForest

                if isinstance(rf, (GpuForestModel, Forest)):
                    raise ValueError("soft_votes=True needs a scikit-learn forest from the trainer: "
                                     f"{type(rf).__name__} keeps no leaf distributions")
                forest = ProbabilityForest.from_sklearn(rf)
            else:
                forest = rf.forest if isinstance(rf, GpuForestModel) else \
                    Forest.from_sklearn(rf, multiclass=True) if multiclass or strategy == "information_density" \
                    else Forest.from_sklearn(rf)
            if strategy == "uncertainty":
                from .uncertainty_sampling import select
                sel = select(state, unlabeled, forest, k)
            elif bald:
                from .uncertainty_sampling import select
                sel = select(state, unlabeled, forest, k, strategy="bald")
            elif strategy == "ranked_batch":
                from .uncertainty_sampling import select_batch
                sel = select_batch(state, unlabeled, lab, forest, k, alpha=alpha, sim_pool=sim_pool)
            elif strategy == "density":
                from .density_weighting import select
                sel = select(state, unlabeled, forest, k, beta=beta)
            elif strategy == "information_density":
                from .density_weighting import select_multiclass
                sel = select_multiclass(state, unlabeled, forest, k, beta=beta)
            elif soft_density:
                from .density_weighting import select_soft
                sel = select_soft(state, unlabeled, forest, k, beta=beta)
            elif strategy == "lal":
                from .active_learner import select_lal
                sel = select_lal(state, unlabeled, forest, lal_model, k, n_labeled=len(labeled),
                                 n_positive=int(np.asarray(y)[lab].sum()))
            else:
                raise ValueError(f"unknown strategy {strategy!r}")
            chosen = sel.indices.cpu().numpy()
            if density_over == "unlabeled":
                state.exclude(chosen)  # the next step's E is the current labeled set
        res.labeled_history.append(chosen)
        res.accuracy.append(acc)
        labeled.extend(int(i) for i in chosen)
        unlabeled = np.setdiff1d(unlabeled, chosen, assume_unique=True)
        line = f"Iteration  {it}  -- accu =  {acc}"
        res.log.append(line)
        if verbose:
            print(line)
        it += 1
    return res
