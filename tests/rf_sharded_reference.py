"""Test-side, level-stepped restatement of the three forest trainers: the
local half of a row-sharded fit (dal.parallel.train_classifier /
train_regressor, the ``steps`` argument) in numpy and Python integers.

A level is two steps, as on the device: the integer statistics of the shard's
rows (class counts per node and per (node, slot, bin) for the classifiers;
(count, limbs of y, limbs of fl(y y)) words for the regressor), then -- from
the statistics summed over the shards -- leaf or best split per node.  The
arithmetic is the existing references':

  thresholds, bins   oracle.rf_oracle.find_splits, bin_values
  Gini, gain, leaf   rf_multiclass_reference.gini, impurity_stats, predict
                     (at two classes the oracle's arithmetic)
  variance           rf_regress_reference.variance over exact sums: a sum is a
                     Python integer in units of 2^q, rounded once
                     (math.ldexp(float(total), q), Dyadic.to_float's rounding)

so a sharded fit through these steps must equal the references' one-piece
fits of the concatenated rows byte for byte."""
import math
from fractions import Fraction

import numpy as np
import torch

import rf_multiclass_reference as RM
import rf_regress_reference as RR
from oracle.rf_oracle import INVALID_GAIN, bin_values, find_splits

LIMB = 31


def to_units(v: float, q: int) -> int:
    """The finite double v as an integer multiple of 2^q (q at or below its lowest set bit)."""
    f = Fraction(float(v)) / (Fraction(2) ** q)
    assert f.denominator == 1, (v, q)
    return int(f)


def to_words(total: int, k: int):
    """A Python integer as k signed words, 31 bits each but the last (which holds the rest)."""
    sign, mag = (-1 if total < 0 else 1), abs(total)
    words = [sign * ((mag >> (LIMB * j)) & ((1 << LIMB) - 1)) for j in range(k - 1)]
    words.append(sign * (mag >> (LIMB * (k - 1))))
    assert all(abs(w) < 1 << 63 for w in words)
    return words


def from_words(words) -> int:
    return sum(int(w) << (LIMB * j) for j, w in enumerate(words))


class NumpySteps:
    """One shard's job; the methods dal.random_forest.HipSteps documents."""

    def rows(self, x_local, regress):
        x = np.asarray(x_local)
        keep = regress and x.dtype == np.float64
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64 if keep else np.float32))

    def find_splits(self, sample, ns, regress):
        s = sample.numpy().astype(np.float64)
        thr = [find_splits(s[:, f], ns) for f in range(s.shape[1])]
        return thr, np.array([t.size for t in thr], dtype=np.int64), torch.zeros(1, dtype=torch.int32)

    def begin(self, job):
        self.j = j = job
        x = j.x.numpy().astype(np.float64)
        n, d = x.shape
        self.bins = np.stack([bin_values(x[:, f], j.thresholds[f]) for f in range(d)], axis=1) if n else \
            np.zeros((0, d), dtype=np.int64)
        self.w = np.asarray(j.weights, dtype=np.int64)
        self.T = T = self.w.shape[0]
        self.hb = j.ns + 2
        n_inner = (1 << j.max_depth) - 1
        self.node = np.zeros((T, n), dtype=np.int64)
        self.open = [{0: False} for _ in range(T)]  # per tree: heap index -> preset leaf flag
        self.sf = np.full((T, n_inner), -1, dtype=np.int64)
        self.sb = np.zeros((T, n_inner), dtype=np.int64)
        if j.regress:
            q_y, k_y, q_sq, k_sq = j.fmt
            self.W = 1 + k_y + k_sq
            y = [float(v) for v in j.y]
            self.iy = [to_units(v, q_y) for v in y]
            self.iq = [to_units(v, q_sq) for v in RR.squares(y)]
            self.leaf = np.zeros((T, n_inner + 1), dtype=np.float64)
        else:
            self.W = int(j.num_classes)
            self.leaf = np.zeros((T, n_inner + 1), dtype=np.uint8)

    def _cell(self, i, w):
        """Row i's contribution to a cell, as W integers."""
        if not self.j.regress:
            v = [0] * self.W
            v[int(self.j.y[i])] = w
            return v
        _, k_y, _, k_sq = self.j.fmt
        return [w] + to_words(w * self.iy[i], k_y) + to_words(w * self.iq[i], k_sq)

    def level_stats(self, level):
        j, W, hb = self.j, self.W, self.hb
        nodes, first = 1 << level, (1 << level) - 1
        tot = np.zeros((self.T, nodes, W), dtype=object)
        hist = np.zeros((self.T, nodes, j.m, hb, W), dtype=object) if level < j.max_depth else None
        tot[...] = 0
        if hist is not None:
            hist[...] = 0
        for t in range(self.T):
            for i in np.nonzero(self.w[t] > 0)[0]:
                if level > 0:
                    hp = self.node[t, i]
                    if hp < 0:
                        continue
                    f = self.sf[t, hp]
                    if f < 0:  # the row's node became a leaf
                        self.node[t, i] = -1
                        continue
                    self.node[t, i] = 2 * hp + 1 + (1 if self.bins[i, f] > self.sb[t, hp] else 0)
                h = int(self.node[t, i])
                cell = self._cell(i, int(self.w[t, i]))
                for k in range(W):
                    tot[t, h - first, k] += cell[k]
                if hist is None or self.open[t].get(h, True):
                    continue
                for s, f in enumerate(j.subsets[t, h]):
                    b = int(self.bins[i, int(f)])
                    for k in range(W):
                        hist[t, h - first, s, b, k] += cell[k]
        flat = np.concatenate([tot.ravel()] + ([] if hist is None else [hist.ravel()]))
        return torch.from_numpy(flat.astype(np.int64)).to(torch.int64 if j.regress else torch.int32)

    def _stats(self, words):
        """(count, impurity, leaf value) of a cell of summed words (Python integers)."""
        if not self.j.regress:
            return int(sum(words)), RM.gini(words), RM.predict(words)
        q_y, k_y, q_sq, _ = self.j.fmt
        c = int(words[0])
        s = math.ldexp(float(from_words(words[1:1 + k_y])), q_y)
        sq = math.ldexp(float(from_words(words[1 + k_y:])), q_sq)
        return c, RR.variance(c, s, sq), (s / float(c) if c else 0.0)

    def split(self, level, reduced):
        j, W, hb = self.j, self.W, self.hb
        nodes, first = 1 << level, (1 << level) - 1
        n_inner = (1 << j.max_depth) - 1
        r = [int(v) for v in reduced.numpy()]
        tot = np.array(r[:self.T * nodes * W], dtype=object).reshape(self.T, nodes, W)
        hist = np.array(r[self.T * nodes * W:], dtype=object).reshape(self.T, nodes, j.m, hb, W) \
            if level < j.max_depth else None
        for t in range(self.T):
            nxt = {}
            for h, preset_leaf in sorted(self.open[t].items()):
                total = list(tot[t, h - first])
                tc, parent_imp, value = self._stats(total)
                best_gain, best = INVALID_GAIN, None
                if not preset_leaf and level < j.max_depth:
                    for s, f in enumerate(j.subsets[t, h]):
                        f = int(f)
                        left = [0] * W
                        for k in range(int(j.n_splits[f])):
                            left = [a + b for a, b in zip(left, hist[t, h - first, s, k])]
                            right = [a - b for a, b in zip(total, left)]
                            if j.regress:
                                lc, li, _ = self._stats(left)
                                rc, ri, _ = self._stats(right)
                                if lc < j.min_instances or rc < j.min_instances:
                                    continue
                                gain = parent_imp - (lc / float(tc)) * li - (rc / float(tc)) * ri
                                if gain < j.min_gain:
                                    continue
                            else:
                                gain, li, ri = RM.impurity_stats(left, right, parent_imp, j.min_instances,
                                                                 j.min_gain)
                            if gain > best_gain:
                                best_gain, best = gain, (f, k, li, ri)
                if preset_leaf or level == j.max_depth or best_gain <= 0:
                    span = 1 << (j.max_depth - level)
                    lo = (h + 1) * span - 1 - n_inner
                    self.leaf[t, lo:lo + span] = value
                    continue
                f, k, li, ri = best
                self.sf[t, h], self.sb[t, h] = f, k
                child_leaf = level + 1 == j.max_depth
                nxt[2 * h + 1] = child_leaf or li == 0.0
                nxt[2 * h + 2] = child_leaf or ri == 0.0
            self.open[t] = nxt

    def finish(self):
        thr = np.full(self.sf.shape, np.nan if not self.j.regress else np.inf)
        for t, h in zip(*np.nonzero(self.sf >= 0)):
            thr[t, h] = self.j.thresholds[self.sf[t, h]][self.sb[t, h]]
        if self.j.regress:
            return np.where(self.sf >= 0, self.sf, 0).astype(np.int32), thr, self.leaf
        return RM.heap_arrays(self.sf, thr, self.leaf)


def split_shards(X, y, parts):
    """[(x, y, positions)] for a list of position arrays."""
    return [(X[p], y[p], p) for p in (np.asarray(p, dtype=np.int64) for p in parts)]


def contiguous(n, sizes):
    assert sum(sizes) == n
    edges = np.cumsum([0] + list(sizes))
    return [np.arange(a, b) for a, b in zip(edges[:-1], edges[1:])]


def interleaved(n, P, empty=None):
    """Position i goes to the i-th of the non-empty ranks in turn."""
    live = [r for r in range(P) if r != empty]
    return [np.arange(n)[np.arange(n) % len(live) == live.index(r)] if r in live else np.zeros(0, dtype=np.int64)
            for r in range(P)]
