"""Uncertainty sampling query step -- drop-in for final_thesis/uncertainty_sampling.py.

The reference's loop body (uncertainty_sampling.py:85-112) runs T Spark jobs of
``DecisionTreeModel(tree).predict`` over the unlabeled pool (:88-93), sums the
hard votes per row (:96-97), scores ``abs(0.5 - (1 - v/T))`` (:98), sorts
ascending (:106) and takes ``window_size`` rows (:109).  Here that is one
fused HIP kernel (votes + fp64 LUT score + sort key) and a device top-k.
Scores are attached to their own rows (the intended alignment of
lal_direct_mllib_implementation/classes/active_learner.py:160-183; the script's
positional re-key at :100-104 mis-aligns rows when Spark shuffles).
Ties (frequent: only T+1 distinct scores) go to the lower pool index.
"""
from __future__ import annotations

from .engine import PoolState, Selection, as_pool_state, multiclass_step, soft_step, uncertainty_step
from .forest import Forest, ProbabilityForest
from .luts import STRATEGIES


def _check_strategy(strategy: str, forest):
    """The three strategies, and "bald" for a ProbabilityForest alone (a
    hard-voting Forest keeps no leaf distributions); before any work."""
    if strategy == "bald":
        if not isinstance(forest, ProbabilityForest):
            raise ValueError("strategy='bald' (the trees' disagreement) needs a ProbabilityForest (soft votes): a "
                             "hard-voting Forest keeps no leaf distributions")
    elif strategy not in STRATEGIES:
        raise ValueError(f"strategy must be one of {STRATEGIES}")


def select(pool, unlabeled_idx, forest: Forest, k: int, strategy: str = "least_confidence",
           device=None) -> Selection:
    """Score every unlabeled row and select the k most uncertain.

    pool           [N, D] fp32 (numpy or torch; or a PoolState to reuse caches)
    unlabeled_idx  global row indices of the unlabeled set
    forest         dal.forest.Forest (from_sklearn / from_nodes / synthetic)
    k              batch size (``window_size``; clamped to the unlabeled count)
    strategy       "least_confidence" (reference), "margin" or "entropy"
    Returns Selection(scores[U], indices[k], selected_scores[k], votes[U]).

    A multiclass forest (``forest.n_classes`` > 2, at most 32 classes and 255
    trees) is scored by the C-class forms of the three strategies
    (dal.luts.multiclass_lut): the Selection then carries ``counts`` [U, C]
    and ``votes`` is None.

    A dal.forest.ProbabilityForest (soft votes: the averaged leaf class
    distributions, scikit-learn's ``predict_proba``) is scored by the same
    three strategies on the averaged probabilities, exactly
    (dal.engine.soft_step): the Selection then carries ``sums`` [U, C] and
    ``proba()``; ``votes`` and ``counts`` are None.  Such a forest alone also
    takes strategy "bald": the trees' disagreement H(pbar) - mean_t H(p_t)
    (the mean KL divergence to the consensus; query by committee), largest
    first, with ``entropy`` [U] and ``hsum`` [U] beside the sums.  A
    hard-voting Forest raises ValueError for it.
    """
    _check_strategy(strategy, forest)
    state = as_pool_state(pool, device=device)
    if isinstance(forest, ProbabilityForest):
        return soft_step(state, unlabeled_idx, forest, k, strategy)
    if forest.n_classes > 2:
        return multiclass_step(state, unlabeled_idx, forest, k, strategy)
    return uncertainty_step(state, unlabeled_idx, forest, k, strategy)


def select_batch(pool, unlabeled_idx, labeled_idx, forest: Forest, k: int, strategy: str = "least_confidence",
                 alpha=None, sim_pool=None, device=None) -> Selection:
    """Ranked batch-mode uncertainty sampling (Cardoso et al. 2017; modAL's
    batch uncertainty sampling): the k picks of
    dal.similarity.ranked_batch_select with the forest's uncertainty as the
    weight, so a batch is spread over the pool instead of being the first k
    rows of the top tie group.

    The votes (binary) or per-class counts and scores (multiclass) come from
    the score entries ``select`` uses.  Weights in [0, 1], higher = more
    uncertain: binary, dal.luts.batch_weight_lut(strategy, T) gathered by the
    votes; multiclass and soft votes (a ProbabilityForest),
    dal.luts.batch_weights_multiclass of the scores ("bald", a
    ProbabilityForest only: score / log2(C) capped at 1, the entropy rule).  They
    are scattered to pool rows on the device; the candidates are the unlabeled
    rows, the comparison set starts as ``labeled_idx`` (at least one row).

    sim_pool: the bf16 [N, 64|128|256] matrix the cosines are taken on (e.g. an
    embedding of the pool); None: the pool itself rounded to bf16 -- ValueError
    at other widths.  alpha: see ranked_batch_select (one number per call;
    None: U / (U + labeled count)).  The whole pool on one device (no shard).

    Returns Selection(scores = fp32 max-cosine of the unlabeled rows after the
    last pick, indices, selected_scores = the fp64 ranked scores at pick time)
    with ``selected_similarity``, ``weights`` (fp64 [U]) and ``votes`` /
    ``counts`` as ``select`` returns them."""
    import torch

    from . import luts
    from .engine import _as_index
    from .similarity import _bf16_pool, ranked_batch_select

    _check_strategy(strategy, forest)
    state = as_pool_state(pool, device=device)
    if state.row_base or state.n_total != state.n:
        raise ValueError("select_batch needs the whole pool, not a row shard")
    dev = state.device
    if sim_pool is None:
        if getattr(state, "_sim_bf16", None) is None:
            state._sim_bf16, _ = _bf16_pool(state.x, dev)  # (rounded once per pool)
        simx = state._sim_bf16
    else:
        simx, _ = _bf16_pool(sim_pool, dev)
        if simx.shape[0] != state.n:
            raise ValueError("sim_pool must have one row per pool row")
    unl = _as_index(unlabeled_idx, dev)
    scored = select(state, unl, forest, 1, strategy)  # votes / counts and scores of every unlabeled row
    if forest.n_classes > 2 or isinstance(forest, ProbabilityForest):
        w_unl = luts.batch_weights_multiclass(strategy, scored.scores, forest.n_classes)
    else:
        table = torch.from_numpy(luts.batch_weight_lut(strategy, forest.n_trees)).to(dev)
        w_unl = table[scored.votes.to(torch.int64)]
    weights = torch.zeros(state.n, dtype=torch.float64, device=dev)
    weights[unl] = w_unl
    ranked = ranked_batch_select(simx, labeled_idx, weights, k, alpha=alpha, candidates=unl, device=dev)
    sel = Selection(scores=ranked.scores, indices=ranked.indices, selected_scores=ranked.selected_scores,
                    votes=scored._votes, counts=scored._counts, sums=scored._sums,
                    denominator=scored.denominator, entropy=scored._entropy, hsum=scored._hsum)
    sel.selected_similarity = ranked.selected_similarity
    sel.weights = w_unl
    return sel


__all__ = ["select", "select_batch", "PoolState", "Selection"]
