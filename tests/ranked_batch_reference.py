"""Ranked batch-mode selection restated in numpy: the canonical definition of
include/dal.h (dal_kcenter_ranked_*) on top of tests/kcenter_reference.py's
canonical cosine, the vote-weighted clustered pools the tests share, and the
local half of the sharded selection (the ranked methods of
dal.similarity.HipKCenterSteps) without a GPU.

Every operation is one numpy fp64 operation in the header's order: b = 1 -
alpha, c = b * w, g = alpha * (1 - m) + c."""
import numpy as np
import torch

import kcenter_reference as KR
from oracle import dal_oracle as O

SHAPES = [(2000, 64, 20, 8, 60), (1500, 128, 16, 4, 16), (1200, 256, 12, 5, 40)]  # n, d, clusters, m, k
T = 10


def default_alpha(n_candidates, m):
    return n_candidates / (n_candidates + m)


def _live(n, candidates):
    live = np.zeros(n, dtype=bool)
    if candidates is None:
        live[:] = True
    else:
        c = np.asarray(candidates, dtype=np.int64)
        live[c[(c >= 0) & (c < n)]] = True
    return live


def _score(alpha, m, c):
    return np.float64(alpha) * (1.0 - m) + c


def ranked_reference(X, L, w, k, alpha=None, candidates=None):
    """(picks int64 [kk], scores s_t fp64 [kk], similarities r_t fp64 [kk],
    final m fp64 [n]) of the ranked batch-mode rule."""
    X = np.asarray(X, dtype=np.float32)
    n = X.shape[0]
    U = O.l2_normalize(X)
    m, _ = O.max_cosine_canonical(X, L)
    live = _live(n, candidates)
    if alpha is None:
        alpha = default_alpha(int(live.sum()), len(L))
    c = (1.0 - np.float64(alpha)) * np.asarray(w, dtype=np.float64)
    picks, scores, sims = [], [], []
    for _ in range(min(int(k), int(live.sum()))):
        g = _score(alpha, m, c)
        p = int(np.argmax(np.where(live, g, -np.inf)))  # the first maximum: the lowest index
        picks.append(p)
        scores.append(g[p])
        sims.append(m[p])
        live[p] = False
        m = np.maximum(m, KR.cos_to(U, U[p]))
    return (np.asarray(picks, dtype=np.int64), np.asarray(scores, dtype=np.float64),
            np.asarray(sims, dtype=np.float64), m)


def runner_up_gaps(X, L, w, k, alpha, candidates=None):
    """Per step, g of the pick minus g of the best other live candidate."""
    X = np.asarray(X, dtype=np.float32)
    U = O.l2_normalize(X)
    m, _ = O.max_cosine_canonical(X, L)
    live = _live(X.shape[0], candidates)
    c = (1.0 - np.float64(alpha)) * np.asarray(w, dtype=np.float64)
    gaps = []
    for _ in range(min(int(k), int(live.sum()))):
        g = np.where(live, _score(alpha, m, c), -np.inf)
        p = int(np.argmax(g))
        live[p] = False
        gaps.append(g[p] - np.where(live, g, -np.inf).max())
        m = np.maximum(m, KR.cos_to(U, U[p]))
    return np.asarray(gaps)


def cluster_votes(n, clusters):
    """Vote counts of a T = 10 forest that follow the cluster i % clusters: 5 in
    clusters 0-1, 4 or 6 in clusters 2-7, one of 0, 1, 9, 10 elsewhere."""
    i = np.arange(n)
    c, j = i % clusters, i // clusters
    return np.where(c < 2, 5, np.where(c < 8, np.array([4, 6])[j % 2], np.array([0, 1, 9, 10])[j % 4])).astype(np.int64)


def lc_weights(votes, n_trees=T):
    """w = 1 - 2 lc[v], the least-confidence batch weight (dal.luts.batch_weight_lut)."""
    lc = np.array([abs(0.5 - (1 - (v / n_trees))) for v in range(n_trees + 1)])
    return (1.0 - 2.0 * lc)[votes]


def weighted_case(shape):
    """(X, labeled indices, candidates, w) of a shape: tests/kcenter_reference's
    clustered pool, the labeled rows the first m rows of cluster 0."""
    n, d, clusters, m, k = shape
    X = KR.clustered_pool(n, d, clusters, seed=n + d)
    L = np.arange(m, dtype=np.int64) * clusters
    cand = np.setdiff1d(np.arange(n, dtype=np.int64), L)
    return X, L, cand, lc_weights(cluster_votes(n, clusters))


class NumpyRankedSteps(KR.NumpyKCenterSteps):
    """The local half of dal.parallel.ranked_batch_select_sharded in numpy:
    NumpyKCenterSteps with the ranked record (key of -g, global index, g, the
    similarity m in the reserved word, the row)."""

    def prepare(self, x_local, row_base, labeled_rows, candidates, weights=None, alpha=None):
        count = super().prepare(x_local, row_base, labeled_rows, candidates)
        self.w = np.asarray(weights, dtype=np.float64)
        self.alpha = alpha
        self.selected_similarity = None
        return count

    def begin(self, kk):
        super().begin(kk)
        self.sim = np.full(int(kk), np.nan)
        self.c = (1.0 - np.float64(self.alpha)) * self.w

    def propose(self, t):
        rec = np.zeros(4 + self.d // 4, dtype=np.uint64)
        rec[0], rec[1] = KR.KEY_NONE, np.uint64(0xFFFFFFFFFFFFFFFF)
        rec[2] = rec[3] = np.array(np.nan).view(np.uint64)
        if self.live.any():
            g = _score(self.alpha, self.m, self.c)
            p = int(np.argmax(np.where(self.live, g, -np.inf)))
            rec[0] = KR.score_key(-g[p])
            rec[1] = np.uint64(p + self.base)
            rec[2] = np.array(g[p]).view(np.uint64)
            rec[3] = np.array(self.m[p]).view(np.uint64)
            rec[4:] = KR.bf16_bits(self.X[p]).view(np.uint64)
        return torch.from_numpy(rec.view(np.int64))

    def commit(self, t, records):
        super().commit(t, records)
        if self.idx[t] >= 0:
            R = records.cpu().numpy().view(np.uint64)
            win = [r for r in R if r[0] != KR.KEY_NONE and int(np.int64(r[1])) == self.idx[t]][0]
            self.sim[t] = np.array(win[3]).view(np.float64)

    def finish(self):
        out = super().finish()
        self.selected_similarity = torch.from_numpy(self.sim[:out[0].shape[0]].copy())
        return out
