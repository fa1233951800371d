"""NumPy restatement of PoolState.exclude's bookkeeping (no GPU): which rows
are new to E, which 256-row chunks of the canonical column-sum partials a
batch touches, and the column sum of E u Delta reached by rewriting ONLY those
chunks -- the claim being that the repaired partials are the ones a fresh pool
would compute, so their sequential reduction is oracle.column_sum_canonical.
The density itself is restated as the subtraction it is:
d_i(E u Delta) = d_i(E) - sum_{j in Delta} <u_i, u_j>."""
import numpy as np

CHUNK = 256  # DAL_CANON_CHUNK


def new_rows(excluded, rows, n_total):
    """Sorted distinct rows of ``rows`` outside E; ValueError out of range."""
    new = np.unique(np.asarray(rows, dtype=np.int64).reshape(-1))
    if new.size and (new[0] < 0 or new[-1] >= n_total):
        raise ValueError(f"excluded indices must lie in [0, {n_total})")
    return np.setdiff1d(new, np.asarray(excluded, dtype=np.int64), assume_unique=True)


def touched_chunks(new, row_base=0, n_local=None):
    """Local chunk ids (ascending, distinct) holding a row of ``new`` in the
    shard [row_base, row_base + n_local)."""
    new = np.asarray(new, dtype=np.int64)
    if n_local is not None:
        new = new[(new >= row_base) & (new < row_base + n_local)]
    return np.unique((new - row_base) // CHUNK)


def chunk_partial(U, mask, c):
    """partials[c]: the chunk's non-excluded rows added in row order."""
    acc = np.zeros(U.shape[1], dtype=np.float64)
    for r in range(c * CHUNK, min((c + 1) * CHUNK, U.shape[0])):
        if not mask[r]:
            acc = acc + U[r]
    return acc


def partials(U, mask):
    n_chunks = (U.shape[0] + CHUNK - 1) // CHUNK
    return np.stack([chunk_partial(U, mask, c) for c in range(n_chunks)])


def reduce(parts):
    s = np.zeros(parts.shape[1], dtype=np.float64)
    for c in range(parts.shape[0]):
        s = s + parts[c]
    return s


class Pool:
    """E, its mask and the cached partials of fp64 unit rows U."""

    def __init__(self, U, excluded):
        self.U = np.asarray(U, dtype=np.float64)
        self.n = self.U.shape[0]
        self.excluded = np.unique(np.asarray(excluded, dtype=np.int64))
        self.mask = np.zeros(self.n, dtype=bool)
        self.mask[self.excluded] = True
        self.parts = partials(self.U, self.mask)
        self.rewritten = []  # chunk ids, in the order exclude() rewrote them

    def exclude(self, rows):
        new = new_rows(self.excluded, rows, self.n)
        if new.size == 0:
            return 0
        self.mask[new] = True
        for c in touched_chunks(new):
            self.parts[c] = chunk_partial(self.U, self.mask, c)
            self.rewritten.append(int(c))
        self.excluded = np.union1d(self.excluded, new)
        return int(new.size)

    def colsum(self):
        return reduce(self.parts)


def density_decrement(U, new):
    """sum_{j in new} <u_i, u_j> for every row i (fp64, plain matmul: a
    tolerance reference, not a bit reference)."""
    U = np.asarray(U, dtype=np.float64)
    return U @ U[np.asarray(new, dtype=np.int64)].sum(axis=0)
