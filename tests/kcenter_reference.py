"""Greedy k-center (farthest-first) batch selection restated in numpy: the
canonical definition of include/dal.h (dal_kcenter_*) on top of the oracle's
canonical cosine, a clustered test pool, and the local half of the sharded
selection (the methods of dal.similarity.HipKCenterSteps) without a GPU."""
import numpy as np
import torch

from oracle import dal_oracle as O

KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def cos_to(U, up):
    """cos64 of every unit row of U to the unit row up: sequential over the
    features, multiply then add (max_cosine_canonical's sum)."""
    S = np.zeros(U.shape[0])
    for f in range(U.shape[1]):
        S = S + U[:, f] * up[f]
    return S


def kcenter_reference(X, L, k, candidates=None):
    """(picks int64 [kk] in pick order, pick-time values fp64 [kk], final m
    fp64 [n]) of the greedy k-center rule: m(0) = canonical max-cosine to the
    labeled rows L; each step picks the live candidate with the smallest m
    (ties -> lower index) and then m = max(m, cos64(., pick))."""
    X = np.asarray(X, dtype=np.float32)
    n = X.shape[0]
    U = O.l2_normalize(X)
    m, _ = O.max_cosine_canonical(X, L)
    live = np.zeros(n, dtype=bool)
    if candidates is None:
        live[:] = True
    else:
        c = np.asarray(candidates, dtype=np.int64)
        live[c[(c >= 0) & (c < n)]] = True
    picks, values = [], []
    for _ in range(min(int(k), int(live.sum()))):
        p = int(np.argmin(np.where(live, m, np.inf)))  # the first minimum: the lowest index
        picks.append(p)
        values.append(m[p])
        live[p] = False
        m = np.maximum(m, cos_to(U, U[p]))
    return np.asarray(picks, dtype=np.int64), np.asarray(values, dtype=np.float64), m


def clustered_pool(n, d, clusters, seed, noise=0.05):
    """Gaussian clusters, bf16-rounded: row i belongs to cluster i % clusters."""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((clusters, d))
    X = centers[np.arange(n) % clusters] + noise * rng.standard_normal((n, d))
    return O.bf16_round(X.astype(np.float32))


def score_key(v):
    """The ascending-orderable uint64 key of an fp64 value (csrc/common.hpp score_key)."""
    v = np.float64(v)
    if v == 0.0:
        v = np.float64(0.0)
    b = int(np.array(v).view(np.uint64))
    return np.uint64((~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63))


def bf16_bits(X):
    """The bf16 bit patterns (uint16) of bf16-representable fp32 values."""
    return (np.ascontiguousarray(X, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


class NumpyKCenterSteps:
    """The local half of dal.parallel.kcenter_select_sharded in numpy, with
    the record layout of DAL_KCENTER_RECORD_BYTES(d): key, global index, fp64
    value, one reserved word, the row's d bf16 values -- as int64 words."""

    def prepare(self, x_local, row_base, labeled_rows, candidates):
        X = np.asarray(x_local, dtype=np.float32)
        self.X, self.base = X, int(row_base)
        self.n, self.d = X.shape
        self.U = O.l2_normalize(X)
        UL = O.l2_normalize(np.asarray(labeled_rows, dtype=np.float32))
        self.m = np.full(self.n, -np.inf)
        for ul in UL:
            self.m = np.maximum(self.m, cos_to(self.U, ul))
        self.live = np.zeros(self.n, dtype=bool)
        if candidates is None:
            self.cand = np.arange(self.n)
        else:
            c = np.asarray(candidates, dtype=np.int64) - self.base
            self.cand = c[(c >= 0) & (c < self.n)]  # foreign indices are dropped
        self.live[self.cand] = True
        return torch.tensor([int(self.live.sum())], dtype=torch.int64)

    def begin(self, kk):
        self.idx = np.full(int(kk), -1, dtype=np.int64)
        self.val = np.full(int(kk), np.nan)

    def propose(self, t):
        rec = np.zeros(4 + self.d // 4, dtype=np.uint64)
        rec[0], rec[1] = KEY_NONE, np.uint64(0xFFFFFFFFFFFFFFFF)
        rec[2] = np.array(np.nan).view(np.uint64)
        if self.live.any():
            p = int(np.argmin(np.where(self.live, self.m, np.inf)))
            rec[0] = score_key(self.m[p])
            rec[1] = np.uint64(p + self.base)
            rec[2] = np.array(self.m[p]).view(np.uint64)
            rec[4:] = bf16_bits(self.X[p]).view(np.uint64)
        return torch.from_numpy(rec.view(np.int64))

    def commit(self, t, records):
        R = records.cpu().numpy().view(np.uint64)
        best = None
        for r in R:
            if r[0] != KEY_NONE and (best is None or (r[0], np.int64(r[1])) < (best[0], np.int64(best[1]))):
                best = r
        if best is None:
            return
        g = int(np.int64(best[1]))
        self.idx[t], self.val[t] = g, np.array(best[2]).view(np.float64)
        if 0 <= g - self.base < self.n:
            self.live[g - self.base] = False
        row = (np.ascontiguousarray(best[4:]).view(np.uint16).astype(np.uint32) << 16).view(np.float32)
        self.m = np.maximum(self.m, cos_to(self.U, O.l2_normalize(row[None, :])[0]))

    def finish(self):
        kk = int((self.idx >= 0).sum())
        return (torch.from_numpy(self.idx[:kk].copy()), torch.from_numpy(self.val[:kk].copy()),
                torch.from_numpy(self.m[self.cand]))
