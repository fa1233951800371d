"""fp64 score look-up tables indexed by the integer vote count v in {0..T}.

The reference evaluates these per row in a Python lambda on float64; since v
takes only T+1 values, the product evaluates the same Python float
expressions once per v on the host and the GPU indexes the table.  Keeping the
reference's exact operation order matters: at T=100, 8 of the 50 symmetric vote
pairs of the least-confidence score do NOT tie in fp64 (e.g. v=41 ->
0.09000000000000008, v=59 -> 0.08999999999999997).

  least_confidence  abs(0.5 - (1 - (v/T)))          uncertainty_sampling.py:98,
                                                    active_learner.py:197   (ascending)
  margin            abs((v/T) - (1 - (v/T)))        binary margin            (ascending)
  entropy           -(1-(v/T)) * log2(1-(v/T))      density_weighting.py:148 (descending)
                    v=0 -> -0.0, v=T -> NaN (0 * -inf)
"""
from __future__ import annotations

import math

import numpy as np

STRATEGIES = ("least_confidence", "margin", "entropy")
ASCENDING = {"least_confidence": True, "margin": True, "entropy": False}


def _log2(p: float) -> float:
    # log(x)/log(2) reproduces the reference's printed value for v=1, T=10
    # (0.13680278410054497, results/striatum_distDW_window_10_samples_5000.txt);
    # numpy 2.x log2 differs by one ulp there.
    return math.log(p) / math.log(2)


def lut(strategy: str, n_trees: int) -> np.ndarray:
    T = int(n_trees)
    if T < 1:
        raise ValueError("n_trees must be >= 1")
    if strategy == "least_confidence":
        vals = [abs(0.5 - (1 - (v / T))) for v in range(T + 1)]
    elif strategy == "margin":
        vals = [abs((v / T) - (1 - (v / T))) for v in range(T + 1)]
    elif strategy == "entropy":
        vals = []
        for v in range(T + 1):
            p0 = 1 - (v / T)
            vals.append(-(p0) * _log2(p0) if p0 > 0.0 else float("nan"))
    else:
        raise ValueError(f"unknown strategy {strategy!r}; expected one of {STRATEGIES}")
    return np.array(vals, dtype=np.float64)


# Multiclass forests (C classes, n_c = trees voting class c): one table of
# T + 1 entries per strategy, indexed on the GPU by
#   least_confidence  lc[max_c n_c],               lc[v] = v / T          (ascending)
#   margin            mg[n_(1) - n_(2)],           mg[m] = m / T          (ascending)
#   entropy           sum over c, in class order, of h[n_c],
#                     h[0] = 0.0, h[v] = -(v/T) * log2(v/T)               (descending)
# h[T] is -0.0 and the class-ordered sum starts at +0.0, so no score is NaN.
# New definitions: at C = 2 they are not the binary tables above.
MULTICLASS_ASCENDING = {"least_confidence": True, "margin": True, "entropy": False}


def multiclass_lut(strategy: str, n_trees: int) -> np.ndarray:
    T = int(n_trees)
    if T < 1:
        raise ValueError("n_trees must be >= 1")
    if strategy in ("least_confidence", "margin"):
        vals = [v / T for v in range(T + 1)]
    elif strategy == "entropy":
        vals = [0.0] + [-(v / T) * _log2(v / T) for v in range(1, T + 1)]
    else:
        raise ValueError(f"unknown strategy {strategy!r}; expected one of {STRATEGIES}")
    return np.array(vals, dtype=np.float64)


# Ranked batch-mode selection (dal.similarity.ranked_batch_select) wants a
# weight in [0, 1], higher = more uncertain.  Binary forests: one table of
# T + 1 entries per strategy, Python floats from the tables above,
#   least_confidence  1.0 - 2.0 * lc[v]      lc = lut("least_confidence", T)
#   margin            1.0 - mg[v]            mg = lut("margin", T)
#   entropy           (0.0 + h[T - v]) + h[v], h = multiclass_lut("entropy", T):
#                     the two-term Shannon entropy in class order (class 0 has
#                     T - v votes), 0 at v in {0, T}, 1 at v = T / 2.
# The reference's one-sided entropy score (lut("entropy", T)) is NaN at v = T
# and is not a weight.
def batch_weight_lut(strategy: str, n_trees: int) -> np.ndarray:
    T = int(n_trees)
    if strategy == "least_confidence":
        vals = [1.0 - 2.0 * float(s) for s in lut("least_confidence", T)]
    elif strategy == "margin":
        vals = [1.0 - float(s) for s in lut("margin", T)]
    elif strategy == "entropy":
        h = [float(s) for s in multiclass_lut("entropy", T)]
        vals = [(0.0 + h[T - v]) + h[v] for v in range(T + 1)]
    else:
        raise ValueError(f"unknown strategy {strategy!r}; expected one of {STRATEGIES}")
    return np.array(vals, dtype=np.float64)


def batch_weights_multiclass(strategy: str, scores, n_classes: int):
    """The ranked batch-mode weights of a C-class step from its fp64 scores
    (numpy array or torch tensor; dal.engine.multiclass_step's ``scores``),
    one fp64 operation per row: least_confidence 1 - maxp, margin 1 - margin,
    entropy H / log2(C) with the module's log(x)/log(2), then capped at 1 (the
    uniform vote's quotient can round one ulp above).  "bald" (soft votes: the
    trees' disagreement, dal.engine.soft_step) takes the entropy rule: BALD <=
    H(pbar) <= log2(C)."""
    C = int(n_classes)
    if C < 2:
        raise ValueError("n_classes must be >= 2")
    if strategy in ("least_confidence", "margin"):
        return 1.0 - scores
    if strategy not in ("entropy", "bald"):
        raise ValueError(f"unknown strategy {strategy!r}; expected one of {STRATEGIES}")
    if isinstance(scores, np.ndarray):
        return (scores / _log2(C)).clip(max=1.0)
    # a tensor divisor: dividing a device tensor by a Python float multiplies by its reciprocal
    return (scores / scores.new_full((1,), _log2(C))).clamp(max=1.0)
