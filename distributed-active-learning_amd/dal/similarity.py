"""Pairwise column similarities -- drop-in for final_thesis/similarity.py.

The reference transposes the normalised pool so that points become columns
(:34-37) and calls ``RowMatrix.columnSimilarities()`` (:38): the exact cosine
of every pair i < j (threshold 0, no diagonal).  Returned here as COO arrays
(i, j, value), the fields of the reference's MatrixEntry records.

With a ``threshold`` the call returns only the pairs whose canonical fp64
cosine reaches it (MLlib's ``columnSimilarities(threshold)``, exact here
instead of sampled): an fp16 MFMA filter over the upper triangle of block
pairs with a rigorous error bound, then the candidates inside the bound
re-decided in canonical fp64.  The N x N matrix is never stored, so this form
runs at pool scale.
"""
from __future__ import annotations

import math

from .cosine_similarity import cosine_entries

# Initial candidate capacity of a thresholded call without ``max_pairs``
# (None: min(N (N - 1) / 2, max(2^20, 8 N))); the call retries once with the
# count the first pass reported.
PAIRS_INITIAL_CAP = None


def _split_operand(state):
    """The pool's two-term fp16 split (the filter reads its H runs)."""
    import torch

    from . import _lib
    from .engine import _ptr, _stream

    if state.gram == "sym":
        return state.gram_operand()
    if state._split is None:  # an "f32" pool: split its fp32 unit rows once
        u, _ = state.normalized()
        state._split = torch.empty((state.n_pad, 2 * state.d_pad), dtype=torch.int16, device=state.device)
        _lib.call("dal_split_f16", _ptr(u), state.n_pad, state.d_pad, state.d_pad, _ptr(state._split),
                  _stream(state.device))
    return state._split


def cosine_pair_candidates(state, threshold: float, cap: int, row_blocks=None, col_blocks=None):
    """One filter call (dal_cosine_pairs) on a pool state: (keys int64 [cap],
    approx fp32 [cap], count int64 [1], status int32 [1]) device tensors,
    nothing synchronised.  keys[c] = (i << 32) | j for c < min(count, cap), in
    no particular order.  row_blocks / col_blocks: (first, end) ranges of
    256-row blocks (default: the whole pool); calls whose ranges tile the
    blocks cover every pair exactly once."""
    import torch

    from . import _lib
    from .engine import _ptr, _stream

    dev = state.device
    op = _split_operand(state)
    nb = state.n_pad // 256
    r_lo, r_hi = (0, nb) if row_blocks is None else (int(row_blocks[0]), int(row_blocks[1]))
    c_lo, c_hi = (0, nb) if col_blocks is None else (int(col_blocks[0]), int(col_blocks[1]))
    keys = torch.empty(max(int(cap), 1), dtype=torch.int64, device=dev)
    approx = torch.empty(max(int(cap), 1), dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    flags = _ptr(state.flags) if state.excluded.size else 0
    if r_hi > r_lo and c_hi > c_lo:
        _lib.call("dal_cosine_pairs", _ptr(op) + r_lo * 256 * 2 * state.d_pad * 2, r_lo, r_hi - r_lo, _ptr(op), 0,
                  c_lo, min(c_hi, (state.n + 511) // 512 * 2), state.n, state.d_pad, flags, float(threshold),
                  int(cap), _ptr(keys), _ptr(approx), _ptr(count), _ptr(status), _stream(dev))
    return keys, approx, count, status


def cosine_pair_values(state, keys, n_cand: int):
    """Canonical fp64 cosines of the first ``n_cand`` candidate keys
    (dal_cosine_pairs_resolve)."""
    import torch

    from . import _lib
    from .engine import _ptr, _stream

    values = torch.empty(int(n_cand), dtype=torch.float64, device=state.device)
    if n_cand:
        _lib.call("dal_cosine_pairs_resolve", _ptr(state.x), state.n, state.d, state.d, _ptr(state.norms()),
                  _ptr(keys), int(n_cand), _ptr(values), _stream(state.device))
    return values


def _column_similarities_threshold(pool, threshold, device, max_pairs):
    import torch

    from ._lib import DAL_FLAG_CAND_OVERFLOW
    from .engine import as_pool_state

    try:
        tau = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"threshold must be a finite float in (-1, 1], not {threshold!r}") from None
    if not math.isfinite(tau) or tau <= -1.0 or tau > 1.0:
        raise ValueError(f"threshold must be a finite float in (-1, 1], not {threshold!r}")
    if max_pairs is not None and int(max_pairs) < 0:
        raise ValueError("max_pairs must be >= 0")
    state = as_pool_state(pool, device=device)
    if state.row_base or state.n_total != state.n:
        raise ValueError("column_similarities(threshold=) needs the whole pool, not a row shard")
    n = state.n
    all_pairs = n * (n - 1) // 2
    if max_pairs is not None:
        cap = min(int(max_pairs), all_pairs)
    elif PAIRS_INITIAL_CAP is not None:
        cap = min(int(PAIRS_INITIAL_CAP), all_pairs)
    else:
        cap = min(all_pairs, max(1 << 20, 8 * n))
    _split_operand(state)  # (raises the zero-norm flag into state.status)
    if all_pairs == 0:
        state.check_status()
        return (torch.empty(0, dtype=torch.int64, device=state.device),
                torch.empty(0, dtype=torch.int64, device=state.device),
                torch.empty(0, dtype=torch.float64, device=state.device))
    for attempt in range(2):
        keys, _, count, status = cosine_pair_candidates(state, tau, cap)
        n_cand, st, st_pool = torch.cat([count, status.to(torch.int64), state.status.to(torch.int64)]).tolist()
        state.check_status(st_pool)
        if not (st & DAL_FLAG_CAND_OVERFLOW):
            break
        if max_pairs is not None and n_cand > int(max_pairs):
            raise RuntimeError(f"column_similarities: {n_cand} candidate pairs exceed max_pairs={int(max_pairs)}; "
                               f"pass max_pairs >= {n_cand}")
        if attempt:
            raise RuntimeError(f"column_similarities: candidate count changed between passes ({n_cand} > {cap})")
        cap = n_cand
    values = cosine_pair_values(state, keys, n_cand)
    keep = values >= tau
    kept_keys, order = torch.sort(keys[:n_cand][keep])
    return kept_keys >> 32, kept_keys & 0xFFFFFFFF, values[keep][order]


def column_similarities(pool, threshold=None, device=None, max_pairs=None):
    """(i, j, cos(x_i, x_j)) for every pair i < j, row-major order.

    threshold=None: every pair, from the dense fp32 matrix (small N).

    threshold=tau, a finite float in (-1, 1]: exactly the pairs whose canonical
    fp64 cosine (u = x / ||x|| in fp64, sequential sum over the features,
    multiply then add) is >= tau, as (i int64, j int64, value float64) device
    tensors sorted by (i, j); ``value`` is that canonical cosine.  ``pool`` may
    be an array or a PoolState (its split operand and norms are reused; rows
    of its excluded set appear neither as i nor as j).  ``max_pairs`` bounds
    the filter's candidate count (the returned pairs plus those within about
    2^-10 below tau): exceeding it raises RuntimeError naming the needed count;
    without it the call sizes its buffers itself and retries once."""
    import torch

    if threshold is not None:
        return _column_similarities_threshold(pool, threshold, device, max_pairs)
    if max_pairs is not None:
        raise ValueError("max_pairs applies to a thresholded call")
    S = cosine_entries(pool, device=device)
    n = S.shape[0]
    ij = torch.triu_indices(n, n, offset=1, device=S.device)
    return ij[0], ij[1], S[ij[0], ij[1]]


# ---------------------------------------------------------------------------
# Batch-mode diversity (BASELINE config 5): max-cosine to a labeled set
# ---------------------------------------------------------------------------
def _bf16_pool(pool, device):
    import numpy as np
    import torch

    from .engine import _require_cuda

    dev = _require_cuda(device)
    if isinstance(pool, torch.Tensor):
        x = pool.to(device=dev)
    else:
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(pool, dtype=np.float32))).to(dev)
    if x.dtype != torch.bfloat16:
        x = x.to(torch.float32).to(torch.bfloat16)  # round to nearest even
    if x.dim() != 2 or x.shape[1] not in (64, 128, 256):
        raise ValueError("bf16 max-cosine needs a [rows, 64|128|256] pool")
    return x.contiguous(), dev


class LabeledSet:
    """The labeled rows as the kernels' B operands: bf16 [m_pad, d] (padding
    rows carry 1/||x|| = NaN, ignored by the max) with fp32 1/||x|| for the
    arg-max kernel, the folded fp16 table 2^15 x/||x|| for the max-only
    kernel (``unit16``, built on first use), and the canonical fp64 unit rows
    (feature-major) for the exact re-rank."""

    def __init__(self, rows_bf16, device):
        import torch

        from . import _lib
        from .engine import _ptr, _stream

        lib = _lib.load()
        m, d = int(rows_bf16.shape[0]), int(rows_bf16.shape[1])
        g = int(lib.dal_maxcos_label_rows_granule(d))
        m_pad = -(-m // g) * g
        self.m, self.d, self.m_pad = m, d, m_pad
        self.rows = torch.zeros((m_pad, d), dtype=torch.bfloat16, device=device)
        self.rows[:m] = rows_bf16
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.inv = torch.empty(m_pad, dtype=torch.float32, device=device)
        _lib.call("dal_inv_norms_bf16", _ptr(self.rows), m, m_pad, d, d, _ptr(self.inv),
                  _ptr(self.status), _stream(device))
        # canonical fp64 unit rows, feature-major [d][m] (the re-rank reads
        # them coalesced across labeled rows)
        self.unit64_t = torch.empty((d, m), dtype=torch.float64, device=device)
        _lib.call("dal_canon_unit_rows_bf16", _ptr(self.rows), m, d, d, 1, _ptr(self.unit64_t),
                  _stream(device))
        self.device = device
        self._unit16 = None

    @property
    def unit16(self):
        """fp16 [m_pad, d] = 2^15 x_l / ||x_l|| (canonical fp64 norm, one
        rounding; padding rows repeat row 0) -- dal_max_cosine_unit's B."""
        if self._unit16 is None:
            import torch

            from . import _lib
            from .engine import _ptr, _stream

            u = torch.empty((self.m_pad, self.d), dtype=torch.float16, device=self.device)
            _lib.call("dal_unit_rows_f16", _ptr(self.rows), self.m, self.m_pad, self.d, self.d, _ptr(u),
                      _ptr(self.status), _stream(self.device))
            self._unit16 = u
        return self._unit16


def max_cosine(pool, labeled_idx, device=None):
    """(m, arg): m_i = max_{l in labeled} cos(x_i, x_l) for every pool row
    (fp32 [N]; bf16 MFMA with fp32 accumulation, |error| <=
    dal_maxcos_error_bound(d)) and its arg-max (int32 [N], the position l in
    ``labeled_idx``; the canonical fp64 arg-max, first l on ties -- rows whose
    fp32 top two cannot be ordered are re-ranked exactly in fp64).

    Restates similarity.py:34-38 (columnSimilarities of the normalised pool,
    i.e. every pairwise cosine) reduced to the nearest labeled row."""
    import torch

    from . import _lib
    from .engine import _as_index, _ptr, _stream

    x, dev = _bf16_pool(pool, device)
    n, d = int(x.shape[0]), int(x.shape[1])
    lab = LabeledSet(x[_as_index(labeled_idx, dev)], dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    arg = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.call("dal_max_cosine", _ptr(x), n, d, _ptr(lab.rows), lab.m_pad, _ptr(lab.inv), 0,
              _ptr(out), _ptr(arg), _ptr(status), _stream(dev))
    _lib.call("dal_maxcos_argmax_resolve", _ptr(x), n, d, d, _ptr(lab.unit64_t), lab.m, _ptr(arg),
              _stream(dev))
    if int(status.item()) | int(lab.status.item()):
        raise ValueError("zero-norm row: cosine undefined")
    return out, arg


def diversity_select(pool, labeled_idx, k: int, candidates=None, device=None, row_base: int = 0,
                     labeled_rows=None):
    """Select the k candidate rows least similar to the labeled set (smallest
    max-cosine, ties -> lower index), exact against the canonical fp64
    max-cosine.  Returns Selection(scores = fp32 max-cos of the candidates,
    indices [k], selected_scores = canonical fp64 max-cos).

    The fp32 values come from the folded-operand kernel (dal_max_cosine_unit,
    within dal_maxcos_unit_error_bound(d) ~ 2^-11 of the canonical values, about
    1000x the bf16 kernel's (3d + 6) 2^-24): the bound only widens the interval
    keys, the selection stays exact through the fp64 re-rank.  When the
    candidate list overflows on that bound (near-tied pools: duplicates,
    clusters), the values are recomputed once with the tighter dal_max_cosine
    (d = 64 / 128 / 256) before the capacity grows; ``scores`` then carry that
    kernel's precision.

    For a row shard (multi-GPU) pass ``row_base`` (global index of row 0),
    global ``candidates`` and the labeled set as ``labeled_rows`` ([m, d],
    replicated on every rank) instead of ``labeled_idx``."""
    import numpy as np
    import torch

    from . import _lib
    from ._lib import DAL_ASCENDING, DAL_FLAG_CAND_OVERFLOW, DAL_FLAG_SAMPLE_MISS, DAL_ROW_CANDIDATE
    from .engine import LEVEL1_PASSES, Selection, _as_index, _ptr, _stream, candidate_cap, workspace

    lib = _lib.load()
    x, dev = _bf16_pool(pool, device)
    n, d = int(x.shape[0]), int(x.shape[1])
    if labeled_rows is not None:
        lab_rows, _ = _bf16_pool(labeled_rows, dev)
    else:
        lab_rows = x[_as_index(labeled_idx, dev)]
    lab = LabeledSet(lab_rows, dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    mx = torch.empty(n, dtype=torch.float32, device=dev)
    # values only (no arg-max): the folded-operand kernel; its wider bound
    # only widens the interval keys -- the fp64 re-rank keeps the selection exact
    _lib.call("dal_max_cosine_unit", _ptr(x), n, d, _ptr(lab.unit16), lab.m_pad, _ptr(mx), _ptr(status),
              _stream(dev))
    bound = float(lib.dal_maxcos_unit_error_bound(d))
    tight = False  # the values are the folded kernel's until a candidate overflow asks for the tighter ones
    in_range = None  # device count of the candidates inside this shard (read with the status)
    if candidates is None:
        flags = torch.full((n,), DAL_ROW_CANDIDATE, dtype=torch.uint8, device=dev)
        cand = torch.arange(n, device=dev)
        n_cand = n
    else:
        flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        gidx = _as_index(candidates, dev)
        # the marking kernel also counts the candidates inside this shard
        in_range = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.call("dal_mark_rows_count", _ptr(gidx), int(gidx.shape[0]), int(row_base), n, DAL_ROW_CANDIDATE,
                  _ptr(flags), _ptr(in_range), _stream(dev))
        cand = gidx - row_base if row_base else gidx
        # an upper bound until the status read: global candidates of other
        # shards are not ours (filtered below, off the common path)
        n_cand = int(cand.shape[0])
        if n_cand == 0:
            return Selection(scores=mx[cand], indices=torch.empty(0, dtype=torch.int64, device=dev),
                             selected_scores=torch.empty(0, dtype=torch.float64, device=dev))
    kk = min(int(k), n_cand)
    lo = torch.empty(n, dtype=torch.int64, device=dev)
    hi = torch.empty(n, dtype=torch.int64, device=dev)
    _lib.call("dal_interval_keys_f32", _ptr(mx), n, bound, _ptr(flags), DAL_ASCENDING, _ptr(lo), _ptr(hi),
              _stream(dev))
    cap = candidate_cap(n, kk)
    passes = LEVEL1_PASSES if cap <= _lib.DAL_SORT_CAP_PAYLOAD else 0
    while True:
        wsb = int(lib.dal_maxcos_select_workspace_bytes(n, kk, cap))
        ws, wsp = workspace(wsb, dev)
        out_idx = torch.empty(kk, dtype=torch.int64, device=dev)
        out_sc = torch.empty(kk, dtype=torch.float64, device=dev)
        _lib.call("dal_maxcos_select", _ptr(lo), _ptr(hi), n, kk, int(row_base), _ptr(x), d, d,
                  _ptr(lab.unit64_t), lab.m, cap, passes, wsp, wsb, _ptr(out_idx), _ptr(out_sc), 0,
                  _ptr(status), _stream(dev))
        # one host read for the status words (and the shard's candidate count)
        words = [status, lab.status] + ([in_range] if in_range is not None else [])
        vals = torch.cat(words).tolist()
        st = vals[0] | vals[1]
        if st & 1:
            raise ValueError("zero-norm row: cosine undefined")
        if in_range is not None and vals[2] < n_cand:
            # candidates outside this shard: filter and redo with the true count
            # (kk must not exceed it, or key-NONE rows would fill the list)
            cand = cand[(cand >= 0) & (cand < n)]
            n_cand, in_range = int(cand.shape[0]), None
            if n_cand == 0:
                return Selection(scores=mx[cand], indices=torch.empty(0, dtype=torch.int64, device=dev),
                                 selected_scores=torch.empty(0, dtype=torch.float64, device=dev))
            kk = min(int(k), n_cand)
            cap = candidate_cap(n, kk)
            passes = LEVEL1_PASSES if cap <= _lib.DAL_SORT_CAP_PAYLOAD else 0
            status.zero_()
            continue
        if st & DAL_FLAG_SAMPLE_MISS and passes > 0:  # the fast level 1 overflowed: exact level 1 first
            passes = 0
            status.zero_()
            continue
        if not tight and st & DAL_FLAG_CAND_OVERFLOW:
            # the exact level 1 also holds too many rows within the folded
            # kernel's bound of the boundary: the bf16 kernel's values (bound
            # ~1000x tighter) and their keys -- not for a fast-level-1 miss alone
            # (identical rows: a tighter bound cannot separate them)
            tight = True
            status.zero_()
            _lib.call("dal_max_cosine", _ptr(x), n, d, _ptr(lab.rows), lab.m_pad, _ptr(lab.inv), 0, _ptr(mx), 0,
                      _ptr(status), _stream(dev))
            bound = float(lib.dal_maxcos_error_bound(d))
            _lib.call("dal_interval_keys_f32", _ptr(mx), n, bound, _ptr(flags), DAL_ASCENDING, _ptr(lo), _ptr(hi),
                      _stream(dev))
            continue
        if cap >= n or not (st & DAL_FLAG_CAND_OVERFLOW):
            break
        status.zero_()
        cap = min(n, cap * 4)
        passes = 0
    return Selection(scores=mx[cand], indices=out_idx, selected_scores=out_sc)


# ---------------------------------------------------------------------------
# Greedy k-center (farthest-first) batch selection
# ---------------------------------------------------------------------------
def check_alpha(alpha) -> float:
    """alpha of a ranked batch-mode job as a float in (0, 1]."""
    try:
        a = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"alpha must be a float in (0, 1], not {alpha!r}") from None
    if not (0.0 < a <= 1.0):
        raise ValueError(f"alpha must be a float in (0, 1], not {alpha!r}")
    return a


def default_alpha(n_candidates: int, m: int) -> float:
    """The ranked batch-mode default |C| / (|C| + m), in Python floats from the
    two integers (1.0 without a candidate: no step runs)."""
    n_candidates, m = int(n_candidates), int(m)
    return n_candidates / (n_candidates + m) if n_candidates > 0 else 1.0


class HipKCenterSteps:
    """The local half of a greedy k-center selection on one device: the
    dal_kcenter_* step entries over one row shard.  The single-device
    ``kcenter_select`` and ``dal.parallel.kcenter_select_sharded`` drive the
    same object; tests inject a numpy restatement with these methods:

    prepare(x_local, row_base, labeled_rows, candidates) -> int64 [1] tensor,
        the number of candidates inside this shard (``candidates`` None: every
        row); computes m(0) and the row flags, nothing is read back;
        ``weights`` (fp64, one per row of x_local) and ``alpha`` make it a
        ranked batch-mode job (dal_kcenter_ranked_*); the driver stores the
        default alpha in ``self.alpha`` before begin;
    begin(kk)       the job for kk steps (dal_kcenter_begin, and
        dal_kcenter_ranked_attach when weights were given);
    propose(t)      -> the shard's record of step t, an int64 [w] tensor,
        w = DAL_KCENTER_RECORD_BYTES(d) / 8;
    commit(t, records)  records int64 [P, w], the same on every rank;
    finish()        -> (indices int64 [kk'], selected_scores fp64 [kk'], scores
        fp32 of this shard's candidates after the last pick), kk' = the steps
        that found a candidate; the status words' one host read.  A ranked
        job's scores are s_t; its r_t are left in ``self.selected_similarity``.
    Nothing between begin and finish reads the device."""

    def __init__(self, device=None):
        self.device = device

    def prepare(self, x_local, row_base, labeled_rows, candidates, weights=None, alpha=None):
        import numpy as np
        import torch

        from . import _lib
        from ._lib import DAL_ROW_CANDIDATE
        from .engine import _as_index, _ptr, _stream

        x, dev = _bf16_pool(x_local, self.device)
        self.weights, self.alpha, self.selected_similarity = None, alpha, None
        if weights is not None:
            w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.asarray(weights, dtype=np.float64))
            w = w.to(device=dev, dtype=torch.float64).contiguous()
            if w.dim() != 1 or w.shape[0] != x.shape[0]:
                raise ValueError("ranked batch selection needs one weight per pool row")
            self.weights = w
        lab_rows, _ = _bf16_pool(labeled_rows, dev)
        if lab_rows.shape[0] < 1 or lab_rows.shape[1] != x.shape[1]:
            raise ValueError("k-center needs at least one labeled row of the pool's width")
        self.x, self.dev, self.row_base = x, dev, int(row_base)
        self.n, self.d = int(x.shape[0]), int(x.shape[1])
        n, d = self.n, self.d
        self.lab = lab = LabeledSet(lab_rows, dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.inv = torch.empty(n, dtype=torch.float32, device=dev)
        self.m32 = torch.empty(n, dtype=torch.float32, device=dev)
        if n:
            _lib.call("dal_inv_norms_bf16", _ptr(x), n, n, d, d, _ptr(self.inv), _ptr(self.status), _stream(dev))
            # m(0) from the tight bf16 kernel (values only): within dal_maxcos_error_bound(d)
            _lib.call("dal_max_cosine", _ptr(x), n, d, _ptr(lab.rows), lab.m_pad, _ptr(lab.inv), 0, _ptr(self.m32), 0,
                      _ptr(self.status), _stream(dev))
        if candidates is None:
            self.flags = torch.full((n,), DAL_ROW_CANDIDATE, dtype=torch.uint8, device=dev)
            self.cand = None
            self.n_cand = n
            return torch.tensor([n], dtype=torch.int64, device=dev)
        self.flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        gidx = _as_index(candidates, dev)
        in_range = torch.zeros(1, dtype=torch.int32, device=dev)
        if n and gidx.shape[0]:
            _lib.call("dal_mark_rows_count", _ptr(gidx), int(gidx.shape[0]), self.row_base, n, DAL_ROW_CANDIDATE,
                      _ptr(self.flags), _ptr(in_range), _stream(dev))
        self.cand = gidx - self.row_base if self.row_base else gidx
        self.n_cand = int(gidx.shape[0])  # an upper bound: foreign indices are dropped by the marking
        return in_range.to(torch.int64)

    def begin(self, kk: int, select: bool = False):
        """select: the whole selection from this one host call (dal_kcenter_select)."""
        import ctypes

        import torch

        from . import _lib
        from .engine import _ptr, _stream, workspace

        lib = _lib.load()
        dev, n, d, m = self.dev, self.n, self.d, self.lab.m
        self.kk = kk = int(kk)
        self.out_idx = torch.empty(kk, dtype=torch.int64, device=dev)
        self.out_sc = torch.empty(kk, dtype=torch.float64, device=dev)
        if kk < 1:
            return
        # the centers table [d][m + kk]: the labeled rows' canonical unit rows, then one column per pick
        self.centers = torch.empty((d, m + kk), dtype=torch.float64, device=dev)
        self.centers[:, :m] = self.lab.unit64_t
        wsb = int(lib.dal_kcenter_workspace_bytes(n, d, m, kk))
        self.ws, wsp = workspace(wsb, dev)
        self.job = ctypes.create_string_buffer(_lib.DAL_KCENTER_JOB_BYTES)
        self.record = torch.empty(_lib.kcenter_record_bytes(d) // 8, dtype=torch.int64, device=dev)
        ranked = self.weights is not None
        _lib.call("dal_kcenter_select" if select and not ranked else "dal_kcenter_begin", self.job, _ptr(self.x), n, d,
                  d, self.row_base, _ptr(self.flags), _ptr(self.m32), _ptr(self.inv), _ptr(self.centers), m, kk, wsp, wsb,
                  _ptr(self.out_idx), _ptr(self.out_sc), _ptr(self.status), _stream(dev))
        if ranked:
            rwsb = int(lib.dal_kcenter_ranked_workspace_bytes(n))
            self.rws = torch.empty(rwsb + 256, dtype=torch.uint8, device=dev)  # (kept: c lives here until the last step)
            rwsp = (_ptr(self.rws) + 255) // 256 * 256
            self.out_sim = torch.empty(kk, dtype=torch.float64, device=dev)
            _lib.call("dal_kcenter_ranked_attach", self.job, _ptr(self.weights), check_alpha(self.alpha), rwsp, rwsb,
                      _ptr(self.out_sim), _stream(dev))
            if select:
                _lib.call("dal_kcenter_run", self.job, _stream(dev))

    def propose(self, t: int):
        from . import _lib
        from .engine import _ptr, _stream

        _lib.call("dal_kcenter_propose", self.job, int(t), _ptr(self.record), _stream(self.dev))
        return self.record

    def commit(self, t: int, records):
        from . import _lib
        from .engine import _ptr, _stream

        records = records.to(self.dev).contiguous()
        _lib.call("dal_kcenter_commit", self.job, int(t), _ptr(records), int(records.shape[0]), _stream(self.dev))

    def finish(self):
        import torch

        from ._lib import DAL_FLAG_NONFINITE

        found = (self.out_idx >= 0).sum().to(torch.int32).reshape(1)
        st, st_lab, kk = torch.cat([self.status, self.lab.status, found]).tolist()  # the one host read
        if (st | st_lab) & 1:
            raise ValueError("zero-norm row: cosine undefined")
        if st & DAL_FLAG_NONFINITE:
            raise ValueError("ranked batch selection: a candidate's weight is not a finite number in [0, 1]")
        if self.weights is not None:
            self.selected_similarity = self.out_sim[:kk] if self.kk >= 1 else self.out_sc[:0]
        if self.cand is None:
            scores = self.m32
        else:
            cand = self.cand
            if self.n_cand:  # candidates of other shards are not ours
                cand = cand[(cand >= 0) & (cand < self.n)]
            scores = self.m32[cand]
        return self.out_idx[:kk], self.out_sc[:kk], scores


def kcenter_select(pool, labeled_idx, k: int, candidates=None, device=None, row_base: int = 0, labeled_rows=None):
    """Greedy k-center (farthest-first, the core-set rule) batch selection:
    k times, pick the candidate with the smallest max-cosine to the labeled
    rows AND the picks so far (ties -> lower index), exact against the
    canonical fp64 definition (include/dal.h, dal_kcenter_*).  Equal to k
    successive ``diversity_select(pool, labeled + picks, 1, candidates minus
    picks)`` calls, at one streaming pass over the pool per pick and without
    their bound on the labeled set's growth.

    Same pool contract as ``diversity_select`` (bf16, d in {64, 128, 256}, at
    least one labeled row).  Returns Selection(scores = the fp32 max-cosine of
    the candidates after the last pick, within dal_kcenter_error_bound(d) of
    the canonical values; indices = the min(k, candidates) picks in pick order;
    selected_scores = their canonical fp64 values at pick time,
    non-decreasing).  Candidate indices outside the pool are dropped."""
    from .engine import Selection, _as_index

    if int(k) < 1:
        raise ValueError("k must be >= 1")
    x, dev = _bf16_pool(pool, device)
    if labeled_rows is None:
        labeled_rows = x[_as_index(labeled_idx, dev)]
    st = HipKCenterSteps(dev)
    st.prepare(x, row_base, labeled_rows, candidates)
    st.begin(min(int(k), st.n_cand), select=True)
    idx, sc, scores = st.finish()
    return Selection(scores=scores, indices=idx, selected_scores=sc)


def ranked_batch_select(pool, labeled_idx, weights, k: int, alpha=None, candidates=None, device=None,
                        row_base: int = 0, labeled_rows=None):
    """Ranked batch-mode selection (Cardoso et al. 2017; modAL's batch
    uncertainty sampling), exact against the canonical fp64 definition
    (include/dal.h, dal_kcenter_ranked_*): k times, pick the candidate that
    maximises

        alpha * (1 - max-cosine to the labeled rows and the picks so far)
        + (1 - alpha) * weights[i]

    (ties -> lower index) and add it to the comparison set.  ``weights``: fp64,
    one per pool row, finite and in [0, 1] for every candidate (higher = more
    wanted, e.g. dal.luts.batch_weight_lut gathered by the forest votes); a
    candidate outside that range raises ValueError.  ``alpha`` in (0, 1] is ONE
    number for the whole call; None means |C| / (|C| + m) with |C| the
    candidates inside the pool and m the labeled rows.  It is NOT recomputed
    per pick (modAL re-derives it as the sets change; here the batch is ranked
    under one rule).  alpha = 1 is ``kcenter_select``'s farthest-first batch.

    Same pool contract as ``kcenter_select``.  Returns Selection(scores = the
    fp32 max-cosine of the candidates after the last pick; indices = the
    min(k, |C|) picks in pick order; selected_scores = their fp64 scores at
    pick time, non-increasing) with the extra attribute
    ``selected_similarity``: the picks' canonical max-cosine at pick time."""
    from .engine import Selection, _as_index

    if int(k) < 1:
        raise ValueError("k must be >= 1")
    if alpha is not None:
        alpha = check_alpha(alpha)
    x, dev = _bf16_pool(pool, device)
    if labeled_rows is None:
        labeled_rows = x[_as_index(labeled_idx, dev)]
    st = HipKCenterSteps(dev)
    count = st.prepare(x, row_base, labeled_rows, candidates, weights=weights, alpha=alpha)
    if alpha is None:
        st.alpha = default_alpha(st.n if candidates is None else int(count.item()), st.lab.m)
    st.begin(min(int(k), st.n_cand), select=True)
    idx, sc, scores = st.finish()
    sel = Selection(scores=scores, indices=idx, selected_scores=sc)
    sel.selected_similarity = st.selected_similarity
    return sel


__all__ = ["column_similarities", "cosine_pair_candidates", "cosine_pair_values", "max_cosine", "diversity_select",
           "LabeledSet", "HipKCenterSteps", "kcenter_select", "ranked_batch_select", "check_alpha", "default_alpha"]
