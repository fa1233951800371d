"""The pools and forests of the BALD tests (tests/test_bald_host.py,
tests/test_gpu_bald.py): the shapes of tests/test_gpu_soft.py, fitted the same
way, and the ones the entropy word adds.  Everything is computed once and never
written."""
import functools

import numpy as np

import bald_reference as B
import soft_reference as R
from dal.forest import ProbabilityForest

# name -> (n, d, T, depth, C): the smallest shape that reaches each path of the launcher
CASES = {
    "scalar_ragged": (1037, 30, 10, 4, 3),     # scalar staging, ragged tile, odd C: the word in the padding slot
    "vec4_binary": (1037, 64, 10, 4, 2),       # 16-byte staging, W = 2, even C: the leaf row grows to 4 words
    "dma_persistent": (517, 256, 10, 4, 10),   # LDS-DMA staging on the persistent grid
    "rows_global": (131, 1100, 3, 2, 3),       # rows read from global memory
    "lanes_per_row": (1037, 30, 100, 4, 5),    # several lanes per row: the cross-lane add of the new accumulator
    "widest_one_hot": (259, 8, 255, 3, 32),    # W = 32, C == W; row 0's leaves one-hot: Hs = 0, score +0.0
    "forest_global": (523, 16, 40, 12, 4),     # forest not LDS-resident: words from the [L] array
    "wide_resident": (300, 12, 9, 3, 21),      # W = 32, forest resident, odd C
    "sixteen_lanes": (67, 300, 5, 3, 6),       # 16 lanes per row
    "single_tree": (1037, 30, 1, 4, 3),        # T = 1: every score in [+0.0, 2^-29], some clamped
    "single_row": (1, 30, 10, 4, 3),
    "between_budgets": (300, 16, 10, 8, 2),    # the entropy kernel keeps the forest in LDS, the BALD kernel does not
}
SYNTHETIC = ("widest_one_hot", "forest_global", "between_budgets")
ONE_HOT_CLASS = 7


def fitted(n, d, T, depth, C, seed):
    """A seeded pool and a scikit-learn forest fitted on its first rows (every
    class among them): ragged trees, shallow leaves, real distributions."""
    from sklearn.ensemble import RandomForestClassifier

    rng = np.random.default_rng(seed)
    X = rng.random((max(n, 200), d)).astype(np.float32)
    y = (np.floor(X[:, 0] * C).astype(int) + (X[:, 1] > 0.6)) % C
    y[:C] = np.arange(C)
    rf = RandomForestClassifier(n_estimators=T, max_depth=depth, random_state=0, n_jobs=1).fit(X[:200], y[:200])
    return X[:n], ProbabilityForest.from_sklearn(rf)


@functools.lru_cache(maxsize=None)
def case(name):
    """(X, forest, restatement class sums S, restatement entropy-word sums HS,
    row flags with ~70 % candidates)."""
    n, d, T, depth, C = CASES[name]
    if name == "widest_one_hot":
        X = np.random.default_rng(5).random((n, d)).astype(np.float32)
        F = ProbabilityForest.synthetic(T, depth, d, C, seed=3)
        # the leaf row 0 reaches in every tree becomes one-hot: its entropy word is 0
        hot = [(t, int(l) - t * (1 << depth), ONE_HOT_CLASS) for t, l in enumerate(R.leaf_rows(F, X[:1])[:, 0])]
        F = ProbabilityForest.synthetic(T, depth, d, C, seed=3, one_hot=hot)
    elif name in SYNTHETIC:
        X = np.random.default_rng(6 + depth).random((n, d)).astype(np.float32)
        F = ProbabilityForest.synthetic(T, depth, d, C, seed=4)
    else:
        X, F = fitted(n, d, T, depth, C, seed=100 + d + C)
    assert F.n_trees == T and F.n_classes == C and F.depth <= depth
    flags = (np.random.default_rng(n + d).random(n) < 0.7).astype(np.uint8)
    flags[0] = 1
    flags.setflags(write=False)
    return X, F, R.sums(F, X), B.hsums(F, X), flags
