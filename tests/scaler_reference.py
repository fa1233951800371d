"""Restatement of the exact StandardScaler (include/dal.h) in
Python integers, straight from the raw fp32 values: no limbs, no quanta per
column.  Every fp32 value is an integer multiple of 2^-149, so a column is a
list of Python integers in units of 2^-UNIT and its sums are exact.

  moments(X)          mean = RN(S1 / n), var = RN((n S2 - S1^2) / (n (n - 1)))
                      (0.0 for n == 1), std = sqrt(var)
  transform(...)      numpy fp64, two roundings, then fp32: MLlib 2.1's dense
                      withMean && withStd branch
  start_state(...)    the fixed definition of Dataset.set_start_state
  column_format / shard_cells
                      what dal.parallel.fit_scaler's local steps return, from
                      the exact integers (the CPU stand-in of the kernels)
"""
import math
from fractions import Fraction

import numpy as np

UNIT = 173  # frexp exponent of the smallest fp32 subnormal is -148, its 24-bit integer mantissa ends 24 below


def column_integers(col):
    """The fp32 values of one column as Python integers in units of 2^-UNIT."""
    col = np.asarray(col)
    assert col.dtype == np.float32 and np.isfinite(col).all()
    m, e = np.frexp(col.astype(np.float64))
    mi = (m * 16777216.0).astype(np.int64)  # 24 bits: exact
    return [int(a) << (int(b) - 24 + UNIT) for a, b in zip(mi, e)]


def moments(X):
    """(mean, std) fp64 [d] of fp32 rows X [n, d]."""
    X = np.asarray(X)
    n, d = X.shape
    mean, std = np.zeros(d), np.zeros(d)
    for c in range(d):
        v = column_integers(X[:, c])
        s1, s2 = sum(v), sum(a * a for a in v)
        mean[c] = float(Fraction(s1, n << UNIT))
        if n >= 2:
            num = n * s2 - s1 * s1
            assert num >= 0
            std[c] = math.sqrt(float(Fraction(num, (n * (n - 1)) << (2 * UNIT))))
    return mean, std


def transform(X, mean, std, with_mean=True, with_std=True, dtype=np.float32):
    z = np.asarray(X, dtype=np.float32).astype(np.float64)
    if with_mean:
        z = z - mean
    if with_std:
        nz = std != 0.0
        factor = np.ones_like(std)
        factor[nz] = 1.0 / std[nz]
        z = np.where(nz, z * factor, 0.0)
    return z.astype(dtype)


def start_state(labels, n_start=2, seed=0):
    y = np.asarray(labels)
    positives, negatives = np.flatnonzero(y == 1), np.flatnonzero(y == 0)
    rng = np.random.default_rng(seed)
    pos, neg = rng.permutation(positives), rng.permutation(negatives)
    rest = rng.permutation(np.concatenate([pos[1:], neg[1:]]))
    known = [int(pos[0]), int(neg[0])] + [int(i) for i in rest[:n_start - 2]]
    return np.array(known, dtype=np.int64), rest[n_start - 2:].astype(np.int64)


# ------------------------------------------ the local steps of fit_scaler --
NO_LOW, NO_TOP = 2 ** 31 - 1, -2 ** 31


def column_format(X):
    """(low, top) int32 [d]: the lowest set bit's exponent and (the top bit's
    exponent) + 1 over the nonzero values of each column."""
    X = np.asarray(X)
    d = X.shape[1]
    low, top = np.full(d, NO_LOW, dtype=np.int32), np.full(d, NO_TOP, dtype=np.int32)
    for c in range(d):
        v = [abs(a) for a in column_integers(X[:, c]) if a]
        if v:
            low[c] = min((a & -a).bit_length() - 1 for a in v) - UNIT
            top[c] = max(a.bit_length() for a in v) - UNIT
    return low, top


def digits(value, k):
    """Signed base-2^31 digits of an integer, least significant first."""
    s, a = (-1 if value < 0 else 1), abs(value)
    assert a >> (31 * k) == 0 or k == 0
    return [s * ((a >> (31 * j)) & (2 ** 31 - 1)) for j in range(k)]


def shard_cells(X, q, k1, k2):
    """int64 [d, k1 + k2]: per column the digits of sum x / 2^q and of
    sum x^2 / 2^(2q) -- one valid cell for the shard's exact sums.  A shard's
    sum can need more bits than one value: the top digit takes the rest."""
    X = np.asarray(X)
    d = X.shape[1]
    out = np.zeros((d, k1 + k2), dtype=np.int64)
    for c in range(d):
        v = column_integers(X[:, c])
        for total, shift, k, at in ((sum(v), UNIT + int(q[c]), k1, 0),
                                    (sum(a * a for a in v), 2 * (UNIT + int(q[c])), k2, k1)):
            assert total % (1 << shift) == 0
            t = total >> shift if total >= 0 else -((-total) >> shift)
            s, a = (-1 if t < 0 else 1), abs(t)
            for j in range(k):
                word = (a >> (31 * j)) & (2 ** 31 - 1) if j < k - 1 else a >> (31 * j)
                out[c, at + j] = s * word
    return out
