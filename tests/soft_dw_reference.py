"""Test-side restatement of the soft-vote information density: the entropy of
the averaged leaf class distributions x density (the oracle module is frozen
and knows hard votes only; the class sums and their entropy are
tests/soft_reference.py's).

  S_c(i)   exact integer class sums                         soft_reference.sums
  H_i      class-ordered entropy of S_c / (T 2^31)          soft_reference.scores(.., "entropy")
  d_i      canonical fp64 density, NaN for i in E           oracle.density_canonical
  score_i  H_i * d_i            beta == 1   (one fp64 multiply)
           H_i * pow(d_i, beta) otherwise
  select   descending, NaN last, -0.0 == +0.0, ties to the lower global
           index, take k                                    oracle.select_topk

The device entropy carries the device log2 (within C 2^-49 of H_i, never -0.0
or NaN), so the GPU tests state exactness on the entropy the call returned:
``scores`` and ``select_scores`` take any entropy vector.
"""
import numpy as np

import soft_reference as R
from oracle import dal_oracle as O

KEY_NAN = np.uint64(0xFFFFFFFFFFFFFFFE)
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def entropy(S, T):
    """H_i of class-sum rows (lists of Python ints)."""
    return R.scores(S, T, "entropy")


def scores(H, d, beta=1.0):
    H = np.asarray(H, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    return H * (d if beta == 1.0 else np.power(d, beta))


def select_scores(sc, index, k):
    """(indices, their scores) of the k best: descending, NaN last, -0.0 ==
    +0.0, ties to the lower index."""
    return O.select_topk(np.asarray(sc, dtype=np.float64), np.asarray(index, dtype=np.int64), k, ascending=False)


def select(X, unlabeled_idx, forest, k, beta=1.0, excluded=None, density=None, H=None):
    """One iteration: (scores [U], selected indices, their scores).
    ``density``: the canonical density of every pool row, ``H``: the entropy of
    every pool row (the restatement's, or the one a device call returned), when
    the caller has them already."""
    unl = np.asarray(unlabeled_idx, dtype=np.int64)
    X = np.asarray(X)
    if density is None:
        density = O.density_canonical(X, excluded)
    h = entropy(R.sums(forest, X[unl]), forest.n_trees) if H is None else np.asarray(H, dtype=np.float64)[unl]
    sc = scores(h, np.asarray(density, dtype=np.float64)[unl], beta)
    idx, sel = select_scores(sc, unl, k)
    return sc, idx, sel


def score_key(s):
    """The library's descending score key of fp64 scores as uint64 (smaller =
    better): -0.0 -> +0.0, NaN -> DAL_KEY_NAN."""
    s = np.asarray(s, dtype=np.float64) + 0.0
    b = s.view(np.uint64)
    u = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    return np.where(np.isnan(s), KEY_NAN, ~u)
