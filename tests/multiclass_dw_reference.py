"""Test-side restatement of the multiclass information density: class entropy
x density (the oracle module is frozen and binary; the per-class counts and
the entropy table are tests/multiclass_reference.py's).

  n_c(i)   per-class tree counts                        multiclass_reference.counts
  H_i      s = 0.0; for c in 0..C-1: s = s + h[n_c]     multiclass_reference.scores(.., "entropy")
           (sequential fp64 adds in class order; never NaN, H_i >= +0.0)
  d_i      the canonical fp64 density (NaN for i in E)  oracle.density_canonical
  score_i  H_i * d_i            beta == 1   (one fp64 multiply)
           H_i * pow(d_i, beta) otherwise
  select   descending, NaN last, -0.0 == +0.0, ties to the lower global
           index, take k                                oracle.select_topk

At C = 2 this is the two-term Shannon entropy h[v] + h[T - v], not the
reference script's one-sided -(1-p) log2(1-p) (oracle.lut_entropy).
"""
import numpy as np

import multiclass_reference as R
from oracle import dal_oracle as O

KEY_NAN = np.uint64(0xFFFFFFFFFFFFFFFE)
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def entropy(cnt, T):
    """H_i of count rows [n, C]."""
    return R.scores(np.asarray(cnt), T, "entropy")


def scores(H, d, beta=1.0):
    H = np.asarray(H, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    return H * (d if beta == 1.0 else np.power(d, beta))


def select_scores(sc, index, k):
    """(indices, their scores) of the k best: descending, NaN last, -0.0 ==
    +0.0, ties to the lower index."""
    return O.select_topk(np.asarray(sc, dtype=np.float64), np.asarray(index, dtype=np.int64), k, ascending=False)


def select(X, unlabeled_idx, forest, k, beta=1.0, excluded=None, density=None, cnt=None):
    """One iteration: (scores [U], selected indices, their scores, counts [U, C]).
    ``density``: the canonical density of every pool row, ``cnt``: the counts
    of every pool row, when the caller has them already."""
    unl = np.asarray(unlabeled_idx, dtype=np.int64)
    X = np.asarray(X)
    if density is None:
        density = O.density_canonical(X, excluded)
    c = R.counts(forest, X[unl]) if cnt is None else np.asarray(cnt)[unl]
    sc = scores(entropy(c, forest.n_trees), np.asarray(density, dtype=np.float64)[unl], beta)
    idx, sel = select_scores(sc, unl, k)
    return sc, idx, sel, c


def score_key(s):
    """The library's descending score key of fp64 scores as uint64 (smaller =
    better): -0.0 -> +0.0, NaN -> DAL_KEY_NAN."""
    s = np.asarray(s, dtype=np.float64) + 0.0
    b = s.view(np.uint64)
    u = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    return np.where(np.isnan(s), KEY_NAN, ~u)
