"""Test-side restatement of the canonical soft-vote forest scores, on Python
integers and floats (the oracle module is frozen and knows hard votes only).

A soft forest has T trees (1 <= T <= 255), C classes (2 <= C <= 32) and L
leaves.  Leaf l holds q[l][c] = rint(p[l][c] 2^31), p = value / total in fp64,
one division per class, total the leaf's weights summed in class order;
rounding to even.  A row goes left at a node when x[f] <= thr, thr the fp32
threshold of the device layout (dal.forest rounds fp64 thresholds toward
-inf).

  S_c(i)  = sum_t q[leaf_t(x_i)][c]           a Python int, < 2^39
  M       = T 2^31
  pred(i) = the lowest class holding the largest S_c

  least_confidence  float(max_c S_c) / float(M)                      ascending
  margin            float(S_(1) - S_(2)) / float(M)                  ascending
  entropy           s = 0.0; s = s + h(float(S_c) / float(M)), c = 0..C-1,
                    h(p) = (-p) * log2(p), h(0) = +0.0               descending

Selection: the canonical top-k of given scores -- score in order, -0.0 ==
+0.0, NaN last, ties to the lower index.
"""
import math

import numpy as np

ASCENDING = {"least_confidence": True, "margin": True, "entropy": False}
STRATEGIES = tuple(ASCENDING)
ONE = 1 << 31
KEY_NONE = 0xFFFFFFFFFFFFFFFF


def quantize(value):
    """[[q_c]] (Python ints) of leaf weight rows ``value`` [L, C]."""
    out = []
    for row in np.asarray(value, dtype=np.float64).tolist():
        total = 0.0
        for v in row:
            total = total + v
        out.append([round((v / total) * float(ONE)) for v in row])  # (round(): half to even)
    return out


def leaf_rows(forest, X):
    """Row of the leaf table every tree reaches for every pool row: int64
    [T, n], by the heap walk over forest.inner / forest.leaf_id."""
    X = np.asarray(X, dtype=np.float32)
    n, rows = X.shape[0], np.arange(X.shape[0])
    feat = forest.inner[:, :, 0]
    thr = np.ascontiguousarray(forest.inner[:, :, 1]).view(np.float32)
    n_inner = (1 << forest.depth) - 1
    out = np.empty((forest.inner.shape[0], n), dtype=np.int64)
    for t in range(forest.inner.shape[0]):
        h = np.zeros(n, dtype=np.int64)
        for _ in range(forest.depth):
            left = X[rows, feat[t, h]] <= thr[t, h]
            h = 2 * h + np.where(left, 1, 2)
        out[t] = forest.leaf_id[t, h - n_inner]
    return out


def sums(forest, X):
    """S_c(i) as a list of n lists of C Python ints."""
    lr = leaf_rows(forest, X)
    q = [[int(w) for w in row] for row in forest.leaf_q.tolist()]
    C = int(forest.n_classes)
    out = []
    for i in range(lr.shape[1]):
        s = [0] * C
        for t in range(lr.shape[0]):
            ql = q[int(lr[t, i])]
            for c in range(C):
                s[c] += ql[c]
        out.append(s)
    return out


def pred(S):
    return np.array([s.index(max(s)) for s in S], dtype=np.uint8)  # (index: the first, so the lowest class)


def _h(p):
    return 0.0 if p == 0.0 else (-p) * math.log2(p)


def score(s, T, strategy):
    """One row's score from its class sums (Python ints)."""
    M = float(T * ONE)
    if strategy == "least_confidence":
        return float(max(s)) / M
    top = sorted(s)
    if strategy == "margin":
        return float(top[-1] - top[-2]) / M
    if strategy != "entropy":
        raise ValueError(strategy)
    e = 0.0
    for v in s:
        e = e + _h(float(v) / M)
    return e


def scores(S, T, strategy):
    return np.array([score(s, T, strategy) for s in S], dtype=np.float64)


def proba(S, T):
    M = float(T * ONE)
    return np.array([[float(v) / M for v in s] for s in S], dtype=np.float64)


def score_key(s, ascending):
    """dal's score_key as a Python int: smaller = better, -0.0 == +0.0, NaN
    after every number."""
    if s != s:
        return 0xFFFFFFFFFFFFFFFE
    if s == 0.0:
        s = 0.0
    b = int(np.float64(s).view(np.uint64))
    u = (~b & KEY_NONE) if b >> 63 else (b | (1 << 63))
    return u if ascending else (~u & KEY_NONE)


def keys(sc, flags, ascending):
    """uint64 keys of scores ``sc``: score_key for the rows whose flag carries
    DAL_ROW_CANDIDATE (bit 0), DAL_KEY_NONE otherwise."""
    return np.array([score_key(float(s), ascending) if f & 1 else KEY_NONE for s, f in zip(sc, flags)],
                    dtype=np.uint64)


def topk(sc, index, k, ascending):
    """The canonical top-k of scores ``sc`` (row-aligned with ``index``):
    score in order, NaN last, ties to the lower index; (indices, scores)."""
    index = np.asarray(index, dtype=np.int64)
    order = sorted(range(len(index)), key=lambda j: (score_key(float(sc[j]), ascending), int(index[j])))[:k]
    return index[order], np.asarray(sc, dtype=np.float64)[order]


def select(S, T, strategy, index, k):
    return topk(scores(S, T, strategy), index, k, ASCENDING[strategy])
