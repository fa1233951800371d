"""Test-side restatement of the canonical thresholded column similarities
(the oracle module is frozen; this adds nothing to it but the threshold).

Canonical cosine of rows i, j: u = oracle.l2_normalize(X) (fp64, sequential
norm, divide), then sum_f u_if * u_jf over the features in ascending f,
multiply then add, no FMA -- the definition oracle.max_cosine_canonical uses.
A pair i < j belongs to the result iff that value is >= tau in fp64.
"""
import functools

import numpy as np

from oracle import dal_oracle as O


def canonical_matrix(X):
    """S[i][j] = canonical cosine, every i, j (small n only)."""
    U = O.l2_normalize(X)
    S = np.zeros((U.shape[0], U.shape[0]))
    for f in range(U.shape[1]):
        S = S + U[:, f, None] * U[None, :, f]
    return S


def canonical_values(U, i, j, block=1 << 18):
    """Canonical cosines of the pairs (i[k], j[k]) from the canonical unit rows U."""
    i = np.asarray(i, dtype=np.int64)
    j = np.asarray(j, dtype=np.int64)
    out = np.zeros(i.shape[0])
    for b0 in range(0, i.shape[0], block):
        a, b = U[i[b0:b0 + block]], U[j[b0:b0 + block]]
        s = np.zeros(a.shape[0])
        for f in range(U.shape[1]):
            s = s + a[:, f] * b[:, f]
        out[b0:b0 + block] = s
    return out


def upper_pairs(S, excluded=None):
    """(i, j, v) of every pair i < j in row-major order, rows of ``excluded`` dropped."""
    n = S.shape[0]
    i, j = np.triu_indices(n, 1)
    v = S[i, j]
    if excluded is not None and len(excluded):
        ex = O.exclusion_mask(n, excluded)
        keep = ~(ex[i] | ex[j])
        i, j, v = i[keep], j[keep], v[keep]
    return i, j, v


def threshold_pairs(S, tau, excluded=None):
    i, j, v = upper_pairs(S, excluded)
    keep = v >= tau
    return i[keep], j[keep], v[keep]


def kth_largest(v, k):
    """The k-th largest value (1-based) of v."""
    return np.partition(v, v.shape[0] - k)[v.shape[0] - k]


@functools.lru_cache(maxsize=None)
def pool_reference(n, d, dist, seed=0):
    """(X, S, tau): a synthetic pool, its canonical matrix and the 2,000th
    largest canonical cosine over the pairs i < j.  Shared by the tests; treat
    as read-only."""
    X = O.synthetic_pool(n, d, seed=seed, dist=dist)
    S = canonical_matrix(X)
    _, _, v = upper_pairs(S)
    tau = float(kth_largest(v, 2000))
    S.setflags(write=False)
    return X, S, tau


def filter_emulation(U, d_pad):
    """The filter's operand as numpy: h = fp16(2^12 fp32(u)) / 2^12 per
    component (fp64 array, exact), zero padded to d_pad features."""
    H = (U.astype(np.float32) * np.float32(4096.0)).astype(np.float16)
    h = np.zeros((U.shape[0], d_pad))
    h[:, : U.shape[1]] = H.astype(np.float64) / 4096.0
    return h
