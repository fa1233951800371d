"""Density-weighted uncertainty query step -- drop-in for final_thesis/density_weighting.py.

Reference pipeline:
  proximity matrix  density_weighting.py:58-75  rows L2-normalised (:66), S = U.U^T
                    via BlockMatrix.multiply (:73), N^2 entries pulled to Python (:74-75)
  L0 exclusion      :89-100   entries with i or j in the initial window are dropped once
  per iteration     :136-145  T per-tree predicts + vote sum
                    :148      e = -(1-v/T) log2(1-v/T)
                    :157-161  d_i = sum of the row's remaining S entries (includes j = i)
                    :166-172  score = e * d, descending sortBy, take(window_size)
Here: a fused MFMA Gram row-sum -- fp16 MFMA on a two-term (hi/lo) fp16
split of the unit rows, each symmetric block pair once, plus an exact
closed-form remainder, accumulated in int64 fixed point (S never exists; the density is cached
per pool because the reference's is constant across iterations), a fused
forest + score kernel, and a device top-k whose boundary candidates are
re-ranked in canonical fp64 so the selected set is bit-exact.
``beta`` (declared at :33, unused by the reference) weights d^beta.
"""
from __future__ import annotations

import numpy as np

from ._lib import DAL_MC_MAX_TREES
from .engine import PoolState, Selection, as_pool_state, density_step, multiclass_density_step, soft_density_step
from .forest import Forest, ProbabilityForest


def information_density(pool, excluded_idx=None, device=None, mode: str = "gram"):
    """d_i = sum_{j not in E} cos(x_i, x_j) for every row (fp64, NaN for i in E).

    excluded_idx  E; the reference uses L0 = range(window_size).
    mode          "gram": fused compensated fp16-split MFMA Gram row-sum (the
                  reference's N^2 algorithm, fp32-class: within
                  dal_density_error_bound_sym of canonical);
                  "separable": exact O(N*D) identity, canonical fp64 bits.
    """
    state = as_pool_state(pool, excluded=excluded_idx, device=device)
    d = state.density(mode)
    state.check_status()
    return d


L0 = "L0"  # excluded_idx default: the reference's initial labeled window
# excluded_idx sentinel: E = every row outside ``unlabeled_idx`` -- the density
# over the CURRENT unlabeled pool (rows leave it as they are labeled; the
# reference freezes E at L0).  A PoolState whose E only has to grow takes the
# incremental path (PoolState.exclude), anything else a cold step.
LABELED = "labeled"


def select(pool, unlabeled_idx, forest: Forest, k: int, beta: float = 1.0, excluded_idx=L0,
           density=None, device=None, mode: str = "gram", window_size=None) -> Selection:
    """Score every unlabeled row by entropy x density^beta and select the top k.

    excluded_idx  rows dropped from the density as i and as j.  Default "L0":
                  the reference's initial labeled window range(window_size)
                  (density_weighting.py:89,95-100); for a PoolState the default
                  keeps the state's own excluded set.  None or [] excludes
                  nothing.  LABELED: every row outside ``unlabeled_idx`` (the
                  density over the current unlabeled pool, which the reference
                  does not compute: its E stays L0); a PoolState whose E is a
                  subset of that set grows it with PoolState.exclude -- the
                  cached density is lowered by the new rows' cosine sums
                  instead of being recomputed.
    window_size   the reference's window (L0 = range(window_size)).  Omitted,
                  it is k -- the script takes window_size rows per iteration
                  (:172) -- unless k may be a batch clamped to a short
                  unlabeled set (k >= |unlabeled|), where L0 is ambiguous and
                  window_size must be given.
    density       optional int64 fixed-point density from a previous call
                  (PoolState.density_fixed()); by default the pool's cached one
    mode          "gram" (default, the reference's algorithm on MFMA) or
                  "separable" (exact O(N*D) identity; same selection)

    Binary forests only: the reference's one-sided entropy is a binary score,
    so a multiclass forest (``forest.n_classes`` > 2) raises ValueError.
    """
    if getattr(forest, "n_classes", 2) > 2:
        raise ValueError("density weighting is binary only: the forest has "
                         f"{forest.n_classes} classes (use dal.uncertainty_sampling.select)")
    state = _pool_state(pool, unlabeled_idx, k, excluded_idx, window_size, device)
    return density_step(state, unlabeled_idx, forest, k, beta=beta, density_fixed=density, mode=mode)


def _pool_state(pool, unlabeled_idx, k, excluded_idx, window_size, device) -> PoolState:
    """The pool with the excluded set of select / select_multiclass applied
    (their ``excluded_idx`` and ``window_size`` arguments)."""
    if isinstance(excluded_idx, str) and excluded_idx == LABELED:
        n_total = pool.n_total if isinstance(pool, PoolState) else \
            int(pool.shape[0]) if hasattr(pool, "shape") else len(pool)
        unl = unlabeled_idx.cpu().numpy() if hasattr(unlabeled_idx, "cpu") else np.asarray(unlabeled_idx)
        unl = unl.astype(np.int64).reshape(-1)
        if unl.size and (unl.min() < 0 or unl.max() >= n_total):
            raise ValueError(f"unlabeled indices must lie in [0, {n_total})")
        keep = np.ones(n_total, dtype=bool)
        keep[unl] = False
        labeled = np.nonzero(keep)[0]
        if isinstance(pool, PoolState):
            if np.isin(pool.excluded, labeled, assume_unique=True).all():
                pool.exclude(labeled)  # E only grows: the incremental path
            else:
                pool.set_excluded(labeled)
            return pool
        return as_pool_state(pool, excluded=labeled, device=device)
    if isinstance(excluded_idx, str):
        if excluded_idx != L0:
            raise ValueError(f"excluded_idx must be index-like, None, {L0!r} or {LABELED!r}")
        if isinstance(pool, PoolState):
            excluded_idx = None
        else:
            if window_size is None:
                n_unl = len(unlabeled_idx) if hasattr(unlabeled_idx, "__len__") else None
                if n_unl is not None and int(k) >= n_unl:
                    raise ValueError("k >= the unlabeled count: k may be a clamped batch, so L0 = "
                                     "range(window_size) is ambiguous -- pass window_size (or excluded_idx)")
                window_size = k
            excluded_idx = range(int(window_size))
    elif excluded_idx is None and isinstance(pool, PoolState):
        excluded_idx = []
    return as_pool_state(pool, excluded=excluded_idx, device=device)


def select_multiclass(pool, unlabeled_idx, forest: Forest, k: int, beta: float = 1.0, excluded_idx=L0,
                      density=None, device=None, mode: str = "gram", window_size=None) -> Selection:
    """Score every unlabeled row by class entropy x density^beta and select
    the top k: the C-class information density.

    score_i = H_i * d_i^beta, H_i = sum over the classes c, in class order, of
    -(n_c/T) log2(n_c/T), n_c the trees voting class c (dal.luts.
    multiclass_lut("entropy", T)); d_i the density of ``select``.  Descending,
    NaN last, ties to the lower index; the selection and ``selected_scores``
    are the canonical fp64 ones.  This is a definition of its own, not the
    reference's one-sided -(1-p) log2(1-p) that ``select`` keeps: any forest
    with n_classes >= 2 is scored through the multiclass kernel, and at two
    classes H is the two-term Shannon entropy.  At most 32 classes and 255
    trees.  The other arguments are those of ``select``.  The Selection
    carries ``counts`` ([U, C] per-class votes); ``votes`` is None."""
    forest.check_classes()
    if forest.n_trees > DAL_MC_MAX_TREES:
        raise ValueError(f"a multiclass forest may hold at most {DAL_MC_MAX_TREES} trees, not {forest.n_trees}")
    state = _pool_state(pool, unlabeled_idx, k, excluded_idx, window_size, device)
    return multiclass_density_step(state, unlabeled_idx, forest, k, beta=beta, density_fixed=density, mode=mode)


def select_soft(pool, unlabeled_idx, forest: ProbabilityForest, k: int, beta: float = 1.0, excluded_idx=L0,
                density=None, device=None, mode: str = "gram", window_size=None) -> Selection:
    """Score every unlabeled row by entropy(predict_proba) x density^beta and
    select the top k: modAL's information density over a soft-voting forest.

    score_i = H_i * d_i^beta, H_i the class-ordered entropy of the averaged
    leaf class distributions S_c / (T 2^31) (dal.uncertainty_sampling's
    soft-vote "entropy" score, the same bits); d_i the density of ``select``.
    Descending, NaN last, ties to the lower index; the selection and
    ``selected_scores`` are the canonical fp64 ones on the entropy the device
    computed (within n_classes 2^-49 of the host's).  ``forest`` must be a
    dal.forest.ProbabilityForest; a hard-voting Forest belongs to ``select``
    (binary) or ``select_multiclass``.  The other arguments are those of
    ``select``.  The Selection carries ``sums`` ([U, C] int64) and
    ``proba()``; ``votes`` and ``counts`` are None."""
    if not isinstance(forest, ProbabilityForest):
        raise ValueError("select_soft scores a dal.forest.ProbabilityForest (soft votes): a hard-voting Forest "
                         "belongs to select (binary) or select_multiclass")
    state = _pool_state(pool, unlabeled_idx, k, excluded_idx, window_size, device)
    return soft_density_step(state, unlabeled_idx, forest, k, beta=beta, density_fixed=density, mode=mode)


__all__ = ["information_density", "select", "select_multiclass", "select_soft", "PoolState", "Selection", "L0",
           "LABELED"]
