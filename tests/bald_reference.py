"""Test-side restatement of the soft-vote BALD score (the trees' mutual
information; the mean KL divergence of the trees' leaf distributions to their
average), on Python integers and floats, beside tests/soft_reference.py.

A soft forest has T trees, C classes and leaf words q[l][c] (soft_reference).

  leaf_h[l] = round(H_l 2^29), a Python int below 2^32 (round(): half to even)
              H_l: e = 0.0; e = e + h(float(q[l][c]) / 2.0**31), c = 0..C-1,
              h(p) = (-p) * log2(p), h(0) = +0.0      (soft_reference._h)
  Hs(i)     = sum_t leaf_h[leaf_t(x_i)]               a Python int, < 2^41
  e(i)      = the soft-vote entropy of the row        (soft_reference.score)
  g(i)      = float(Hs) / float(T 2^29)               one division of two exact doubles
  b         = e - g                                   one rounding
  bald(i)   = b if b > 0 else +0.0                    descending

The two LDS budgets of the launcher are restated here as well: which forests
the entropy kernel and the BALD kernel keep resident.
"""
import numpy as np

import soft_reference as R

SHIFT = 29
FOREST_LDS = 65536


def leaf_word(q_row):
    """round(H 2^29) of one leaf's words (Python ints)."""
    e = 0.0
    for w in q_row:
        e = e + R._h(float(w) / 2.0 ** 31)
    return round(e * float(1 << SHIFT))


def leaf_words(forest):
    """[leaf_h[l]] as Python ints."""
    return [leaf_word([int(w) for w in row]) for row in forest.leaf_q.tolist()]


def hsums(forest, X, words=None):
    """Hs(i) as a list of n Python ints."""
    words = leaf_words(forest) if words is None else words
    lr = R.leaf_rows(forest, X)
    return [sum(words[int(lr[t, i])] for t in range(lr.shape[0])) for i in range(lr.shape[1])]


def bald(e, Hs, T):
    """One row's score from its entropy (a float) and its Hs (a Python int)."""
    b = float(e) - float(Hs) / float(T * (1 << SHIFT))
    return b if b > 0 else 0.0


def balds(E, HS, T):
    return np.array([bald(e, hs, T) for e, hs in zip(E, HS)], dtype=np.float64)


def scores(S, HS, T):
    """The all-Python score of every row: class sums S, entropy-word sums HS."""
    return balds(R.scores(S, T, "entropy"), HS, T)


def mean_kl(forest, X):
    """(1/T) sum_t KL(p_t || pbar) of every row, computed directly in fp64 on
    the leaves' own words (p_t = q / 2^31, pbar = their mean)."""
    lr = R.leaf_rows(forest, X)
    p = forest.leaf_q.astype(np.float64) / 2.0 ** 31
    pt = p[lr]  # [T, n, C]
    pbar = pt.mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = np.where(pt > 0, pt * np.log2(pt / pbar[None]), 0.0)
    return term.sum(axis=2).mean(axis=0)


def _round_up(v, m):
    return (v + m - 1) // m * m


def forest_lds_bytes(T, depth, L, C, bald_form):
    """Bytes of the LDS-resident forest: nodes, leaf ids, then the leaf table
    from the next 16-byte boundary, a leaf's row being round2(C) words (entropy
    kernel) or round2(C + 1) words (BALD: the entropy word at column C)."""
    n_inner, n_leaf = (1 << depth) - 1, 1 << depth
    words = (C + (1 if bald_form else 0) + 1) & ~1
    return _round_up(T * (n_inner * 8 + n_leaf * 4), 16) + L * words * 4


def resident(forest, bald_form):
    return forest_lds_bytes(forest.n_trees, forest.depth, forest.n_leaves, forest.n_classes,
                            bald_form) <= FOREST_LDS
