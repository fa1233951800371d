"""Device pipeline of one query-selection step (single GPU / one shard).

Every arithmetic step is a libdal HIP kernel (include/dal.h); torch is used
only for device memory, the current HIP stream and trivial index plumbing.
There is no CPU fallback: without libdal.so or a GPU these functions raise.

Reference loop body being replaced (one ``while True`` iteration):
  uncertainty_sampling.py:85-112   per-tree predict, vote sum, LC score, sortBy, take(k)
  density_weighting.py:58-100      proximity matrix (built once per pool)
  density_weighting.py:133-176     entropy x density, descending sortBy, take(k)
"""
from __future__ import annotations


import weakref

import numpy as np

from . import _lib
from ._lib import (DAL_ASCENDING, DAL_CANON_CHUNK, DAL_DENSITY_EXACT, DAL_DENSITY_FIXED,
                   DAL_DENSITY_NONE, DAL_DESCENDING, DAL_DOWNDATE_MAX_ROWS, DAL_DOWNDATE_TILE, DAL_FIXED_SCALE,
                   DAL_FLAG_CAND_OVERFLOW,
                   DAL_FLAG_SAMPLE_MISS, DAL_FLAG_ZERO_NORM, DAL_MC_ENTROPY, DAL_MC_LEAST_CONFIDENCE,
                   DAL_MC_MARGIN, DAL_MC_MAX_TREES, DAL_ROW_CANDIDATE, DAL_ROW_EXCLUDED,
                   DAL_SORT_CAP_PAYLOAD, DAL_STEP_RESET_STATUS,
                   DAL_STEP_WS_CLEAN, call)
from .forest import Forest
from .luts import ASCENDING, MULTICLASS_ASCENDING, lut as make_lut, multiclass_lut


def _torch():
    import torch

    return torch


def _stream(device=None) -> int:
    torch = _torch()
    return torch.cuda.current_stream(device).cuda_stream


def _raw_stream(device) -> int:
    """The current HIP stream of ``device`` (an indexed torch.device) as an
    integer, without building a Stream object (warm-step host path)."""
    return _torch()._C._cuda_getCurrentRawStream(device.index)


def _ptr(t) -> int:
    return t.data_ptr()


def _require_cuda(device):
    torch = _torch()
    if not torch.cuda.is_available():
        raise _lib.DalError("dal requires a ROCm GPU (torch.cuda.is_available() is False)")
    dev = torch.device(device if device is not None else "cuda")
    if dev.type == "cuda" and dev.index is None:  # pin the index (raw stream / index checks)
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


class Selection:
    """Result of one selection step (all tensors on the pool's device).

    scores          fp64 [U]: score of every unlabeled row, in ``unlabeled`` order
    indices         int64 [k]: selected global row indices, best first
    selected_scores fp64 [k]: their scores (canonical fp64 for density weighting)
    votes           int32 [U]: forest votes for class 1 of every unlabeled row
                    (None for a multiclass step)
    counts          uint8 [U, C]: per-class forest votes of every unlabeled row
                    (a multiclass step; None otherwise)
    lut             fp64 [T+1]: a LAL step (lal_step) also sets this attribute,
                    the regressor's prediction per vote count
    sums            int64 [U, C]: the exact class sums S_c of every unlabeled
                    row (a soft-vote step, soft_step; None otherwise);
                    ``proba()`` gives them over M = T 2^31 as fp64
    entropy         fp64 [U]: the consensus entropy H(pbar) of every unlabeled
                    row (a soft-vote step with strategy="bald"; None otherwise)
    hsum            int64 [U]: the exact sum of the reached leaves' entropy
                    words (strategy="bald"; None otherwise); the score is
                    max(entropy - hsum / (T 2^29), +0.0)

    ``scores`` / ``votes`` / ``counts`` / ``sums`` / ``entropy`` / ``hsum`` may be given as (per-row tensor, positions): they are
    gathered into unlabeled order on first access (the per-row arrays are
    complete in HBM when the step returns; the gather is only a re-layout, so
    a caller that reads just the selection pays no extra launches).
    """

    def __init__(self, scores, indices, selected_scores, votes=None, counts=None, sums=None, denominator=None,
                 entropy=None, hsum=None):
        self._scores = scores
        self.indices = indices
        self.selected_scores = selected_scores
        self._votes = votes
        self._counts = counts
        self._sums = sums
        self.denominator = denominator  # M = T 2^31 of a soft-vote step
        self._entropy = entropy
        self._hsum = hsum

    @staticmethod
    def _gathered(v):
        if isinstance(v, tuple):
            full, pos = v
            return full if pos is None else full[pos]
        return v

    @property
    def scores(self):
        self._scores = self._gathered(self._scores)
        return self._scores

    @property
    def votes(self):
        self._votes = self._gathered(self._votes)
        return self._votes

    @property
    def counts(self):
        self._counts = self._gathered(self._counts)
        return self._counts

    @property
    def sums(self):
        self._sums = self._gathered(self._sums)
        return self._sums

    @property
    def entropy(self):
        self._entropy = self._gathered(self._entropy)
        return self._entropy

    @property
    def hsum(self):
        self._hsum = self._gathered(self._hsum)
        return self._hsum

    def proba(self):
        """fp64 [U, C]: the averaged class probabilities of a soft-vote step,
        (double)S_c / (double)M, one IEEE division per entry."""
        if self._sums is None:
            raise ValueError("proba() belongs to a soft-vote step (a ProbabilityForest)")
        return soft_proba(self.sums, self.denominator)

    def _detach(self):
        """Materialise the per-row arrays now (their source buffers are about
        to be reused: a warm-step graph replay)."""
        self._scores = self._gathered(self._scores)
        self._votes = self._gathered(self._votes)
        self._counts = self._gathered(self._counts)
        self._sums = self._gathered(self._sums)
        self._entropy = self._gathered(self._entropy)
        self._hsum = self._gathered(self._hsum)

    def __iter__(self):
        """Unpacks as the reference-shaped triple (scores, indices, selected_scores)."""
        return iter((self.scores, self.indices, self.selected_scores))

    def __repr__(self):
        return f"Selection(indices={self.indices!r}, selected_scores={self.selected_scores!r})"

    def as_pairs(self):
        """``add_to_labeled_set`` of the reference: a list of (index, score)."""
        return list(zip(self.indices.cpu().tolist(), self.selected_scores.cpu().tolist()))


class PoolState:
    """A device-resident pool and its per-pool caches.

    The reference builds the proximity matrix once per pool and drops the
    initial labeled window L0 from it once (density_weighting.py:58-100), so the
    density is constant across AL iterations; it is computed lazily here and
    cached (the "warm" path), keyed by the excluded set.

    For a row shard (multi-GPU) ``row_base`` is the global index of row 0 and
    ``n_total`` the global pool size.
    """

    def __init__(self, pool, excluded=None, device=None, row_base: int = 0, n_total=None,
                 n_pad=None, gram: str = None, gram_i8=None, gram_fp4=None, prep_fused=None):
        torch = _torch()
        self.gram = _gram_kind(gram)
        dev = _require_cuda(device)
        lib = _lib.load()
        if isinstance(pool, torch.Tensor):
            x = pool.to(device=dev, dtype=torch.float32)
        else:
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(pool, dtype=np.float32))).to(dev)
        if x.dim() != 2:
            raise ValueError("pool must be a 2-D [rows, features] array")
        self.x = x.contiguous()
        self.device = dev
        self.n, self.d = int(x.shape[0]), int(x.shape[1])
        self.row_base = int(row_base)
        self.n_total = int(n_total) if n_total is not None else self.n
        self.n_pad = int(lib.dal_pad_rows(self.n)) if n_pad is None else int(n_pad)
        if self.n_pad < self.n or self.n_pad % 512:
            raise ValueError("n_pad must be a multiple of 512 and >= the row count")
        self.d_pad = int(lib.dal_pad_features(self.d))
        # The int8 form of the "sym" Gram (int8 MFMA row sums of a(H), the rest
        # in closed form: csrc/gram_i8.hpp).  A property of the pool, not of a
        # call: gram_accumulate and gram_residual must agree, on every shard.
        # None: pools of 128-feature slices whose whole split operand exceeds
        # the contiguous schedule's 32 MB; True / False: tests and A/B runs.
        # The fp4 form (e2m1 MFMA row sums of a4(H) over 256-feature slices:
        # csrc/gram_fp4.hpp) takes the int8 form's place where the rule above
        # picks that one and d_pad is a multiple of 256.  An explicit gram_i8
        # (True or False) with gram_fp4=None means no fp4: tests and A/B runs
        # force the other two forms that way.  Both rules read n_total, so
        # every shard agrees.
        i8_given = gram_i8 is not None
        if gram_i8 is None:
            n_all = (self.n_total + 511) // 512 * 512
            gram_i8 = self.gram == "sym" and self.d_pad % 128 == 0 and n_all * 2 * self.d_pad * 2 > GRAM_I8_MIN_BYTES
        elif gram_i8 and (self.gram != "sym" or self.d_pad % 128):
            raise ValueError("gram_i8 needs gram 'sym' and a feature count padded to a multiple of 128")
        if gram_fp4 is None:
            gram_fp4 = bool(gram_i8) and not i8_given and self.d_pad % 256 == 0
        elif gram_fp4 and (self.gram != "sym" or self.d_pad % 256):
            raise ValueError("gram_fp4 needs gram 'sym' and a feature count padded to a multiple of 256")
        elif gram_fp4 and i8_given and gram_i8:
            raise ValueError("gram_i8 and gram_fp4 are two forms of one Gram: force one")
        self.gram_fp4 = bool(gram_fp4)
        self.gram_i8 = bool(gram_i8) and not self.gram_fp4  # (one form runs)
        self._split_i8 = self._split_fp4 = None
        # The fp4 form's one-pass preparation (dal_prep_split_fp4: operand,
        # codes, partials and the residual's sigma sums from one read of the
        # pool; the same bytes as the separate entries, so the rule is about
        # speed only).  None: whole pools on one GPU with enough 256-row chunks
        # to fill the chip; True / False: tests and A/B runs.
        whole = self.row_base == 0 and self.n == self.n_total and self.n_pad == self.nb_active() * 256
        if prep_fused and not (self.gram_fp4 and whole):
            raise ValueError("prep_fused needs the fp4 form on a whole pool (one GPU, the default n_pad)")
        if prep_fused is None:
            prep_fused = self.gram_fp4 and whole and -(-self.n // DAL_CANON_CHUNK) >= PREP_FUSED_MIN_CHUNKS
        self.prep_fused = bool(prep_fused)
        self._sigma_pre = None  # (sigma^H', S^L') of the fused prep, for the residual that follows
        # after exclude(): the column count the cached Gram density summed and the
        # downdates' share of its error bound (density_error); None / 0: a cold density
        self._density_cols = None
        self._downdate_err = 0.0
        # exclude() drops the warm plans (they capture E's flags and bound by
        # value): the first step after it runs eagerly, so a loop that grows E
        # every iteration captures no hipGraph per iteration
        self._excluded_since_step = False
        self.flags = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        self.excluded = np.zeros(0, dtype=np.int64)
        self.set_excluded(excluded)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._u = None
        self._split = None
        self._norm64 = None
        self._density = None
        self._colsum_partials = None
        self._colsum = None
        self._density_exact = None
        self._acc_pre = None  # density accumulator already zeroed by the prep kernel
        self._xb = None  # blocked feature-major copy of x (dal_pool_blocked), built by the first warm step
        self.blocked_copy = True  # False: never build it (saves n x d fp32 of HBM; same bits, slower K2)
        self._us_steps = 0  # uncertainty steps taken on this pool (the blocked copy pays off from the second)
        self._ws_clean = {}   # (n, k, cap) -> workspace whose top-k header is zero (dal_dw_step)
        self.gram_events = None  # list -> (start, end) HIP events around each Gram call
        self.residual_events = []  # (start, end) HIP events around each residual call (with gram_events)
        self.forest_events = None  # list -> (start, end) HIP events around each forest-score call
        self.select_events = None  # list -> (start, end) HIP events around each dal_dw_select call
        # bench only: a callable run after an eager (per-kernel timed) density
        # step with the step's inputs -- it times the fused step's selection
        # launch on its own (bench.time_step_select; single GPU, fast level 1)
        self.step_select_probe = None
        # bench: a GPU spin (torch.cuda._sleep cycles) queued before each timed
        # call's start event, so the call's launches are all submitted before
        # the GPU reaches them -- the events then bracket the device span, not
        # the host's submission gaps between a call's kernels
        self.event_lead_cycles = 0
        # bench: each timed call is issued this many times back to back between
        # its two events (identical, idempotent launches; the event pair's own
        # cost -- a marker and cache release per record -- is amortised)
        self.event_repeat = 1
        self.cap_scale = 1  # re-rank candidate capacity multiplier, kept after an overflow
        self.cap_base = None  # initial re-rank capacity override (tests: force the overflow path)
        self.level1_fast = True  # fast top-k level 1 allowed (cleared after an overflow on this pool)
        self.use_graphs = True  # hipGraph replay of warm steps (tests compare with eager steps)
        self._graphs = {}  # warm-step graphs by (T, depth, k, beta, cap, level-1 passes[, C: a C-class plan])
        self.last_status = 0     # status word read by the last synchronising select

    def clear_caches(self):
        """Drop normalised rows, density, column sums and the blocked copy
        (forces a cold step)."""
        self._u = self._norm64 = self._density = self._colsum = self._colsum_partials = None
        self._split = self._density_exact = self._xb = self._split_i8 = self._split_fp4 = None
        self._sigma_pre = None
        self._graphs = {}
        self._density_cols, self._downdate_err = None, 0.0

    def blocked_pool(self, forest, build: bool = True, multiclass: bool = None):
        """The pool's blocked feature-major copy (dal_pool_blocked) when the
        forest is one the blocked score kernel applies to (it then reads only
        the features the forest tests), else None.  ``multiclass``: the caller
        scores with the C-class kernels (their rule,
        dal_forest_multiclass_blocked_rows, counts the packed counters'
        exchange region in); None: forest.n_classes > 2 -- a two-class forest
        scored by the C-class kernels passes True.  Built on first use
        (``build``) on the current stream and kept with the pool's caches:
        the warm steps build it, the cold step keeps the row-major kernel.
        The copy costs another n x d fp32 (2 GB at config 4): it is skipped
        (the row-major kernel then runs, same bits) when ``blocked_copy`` is
        False or the device lacks that much free memory plus a 1 GiB margin."""
        if self.n == 0 or not self.blocked_copy:
            return None
        lib = _lib.load()
        if multiclass is None:
            multiclass = forest.n_classes > 2
        if multiclass:
            if not lib.dal_forest_multiclass_blocked_rows(self.d, forest.n_trees, forest.depth,
                                                          int(forest.n_classes)):
                return None
        elif not lib.dal_forest_blocked_rows(self.d, forest.n_trees, forest.depth):
            return None
        if self._xb is None and build:
            torch = _torch()
            floats = int(lib.dal_pool_blocked_floats(self.n, self.d))
            free, _ = torch.cuda.mem_get_info(self.device)
            if free < 4 * floats + (1 << 30):
                return None
            xb = torch.empty(floats, dtype=torch.float32, device=self.device)
            call("dal_pool_blocked", _ptr(self.x), self.n, self.d, self.d, _ptr(xb), _stream(self.device))
            self._xb = xb
        return self._xb

    # ------------------------------------------------------------- caches
    def set_excluded(self, excluded):
        """E (global indices): dropped from the density as i and as j
        (density_weighting.py:95-100)."""
        torch = _torch()
        ex = np.unique(np.asarray([] if excluded is None else list(excluded) if isinstance(excluded, range)
                                  else excluded, dtype=np.int64).reshape(-1))
        if ex.size and (ex[0] < 0 or ex[-1] >= self.n_total):
            # the density error bound counts |E| columns: an index outside the
            # pool would make the interval keys (and the exact selection) unsound
            raise ValueError(f"excluded indices must lie in [0, {self.n_total})")
        if np.array_equal(ex, self.excluded) and hasattr(self, "_u"):
            return
        self.excluded = ex
        self.flags.zero_()
        local = ex[(ex >= self.row_base) & (ex < self.row_base + self.n)] - self.row_base
        if local.size:
            self.flags[torch.from_numpy(local).to(self.device)] = DAL_ROW_EXCLUDED
        self._u = self._norm64 = self._density = self._colsum = self._colsum_partials = None
        self._split = self._density_exact = self._split_i8 = self._split_fp4 = None
        self._sigma_pre = None
        self._graphs = {}
        self._density_cols, self._downdate_err = None, 0.0

    def new_excluded(self, rows):
        """The rows of ``rows`` (global indices) not yet in E: sorted, distinct."""
        new = np.unique(np.asarray(list(rows) if isinstance(rows, range) else rows, dtype=np.int64).reshape(-1))
        if new.size and (new[0] < 0 or new[-1] >= self.n_total):
            raise ValueError(f"excluded indices must lie in [0, {self.n_total})")
        return np.setdiff1d(new, self.excluded, assume_unique=True)

    def exclude(self, rows) -> int:
        """Grow E by ``rows`` (global indices; duplicates and members of E are
        ignored) and return how many rows were new.  With a cached "sym" Gram
        density the caches are repaired, not dropped: the density is lowered in
        place by the rows' cosine sums (dal_density_downdate, an N x k product
        instead of a new N^2 Gram; its bound is added to density_error), and
        the row flags, the operands and the column sums become those of a
        fresh pool with E u rows, byte for byte.  Without a cached density, or
        on a gram "f32" pool, this is set_excluded(E u rows).  Removing rows
        from E is not incremental: use set_excluded."""
        new = self.new_excluded(rows)
        if new.size == 0:
            return 0
        if self._density is None or self.gram == "f32":
            self.set_excluded(np.union1d(self.excluded, new))
            return int(new.size)
        if self.row_base or self.n != self.n_total:
            raise ValueError("exclude on a shard: use dal.parallel.exclude")
        for c0 in range(0, int(new.size), DAL_DOWNDATE_MAX_ROWS):
            chunk = new[c0:c0 + DAL_DOWNDATE_MAX_ROWS]
            self.apply_exclude(chunk, self.delta_operand(chunk))
        return int(new.size)

    def _local_of(self, chunk):
        """(positions in ``chunk``, local rows) of the chunk's rows this pool or shard owns."""
        pos = np.nonzero((chunk >= self.row_base) & (chunk < self.row_base + self.n))[0]
        return pos, chunk[pos] - self.row_base

    def delta_operand(self, chunk):
        """The split operand rows of ``chunk`` (sorted new rows of E, at most
        DAL_DOWNDATE_MAX_ROWS) as dal_density_downdate takes them: int16
        [m_pad, 2 * d_pad], row p = the operand row of chunk[p] where this pool
        or shard owns it, zeros elsewhere (another shard's rows, the padding).
        Gathered BEFORE apply_exclude zeroes those rows."""
        torch = _torch()
        m_pad = (int(chunk.size) + DAL_DOWNDATE_TILE - 1) // DAL_DOWNDATE_TILE * DAL_DOWNDATE_TILE
        out = torch.zeros((m_pad, 2 * self.d_pad), dtype=torch.int16, device=self.device)
        pos, loc = self._local_of(chunk)
        if pos.size:
            out[torch.from_numpy(pos).to(self.device)] = self.gram_operand()[torch.from_numpy(loc).to(self.device)]
        return out

    def apply_exclude(self, chunk, delta_ops):
        """One step of exclude(): ``chunk`` (sorted new rows of E) leaves the
        cached density of this pool's or shard's rows; ``delta_ops``: the
        chunk's operand rows (delta_operand; on several GPUs the integer sum
        of every shard's).  Stream-ordered, in this order: the downdate of
        the density in place, EXCLUDED into the flags and zeros into the
        chunk's operand rows, the touched 256-row chunks of the column-sum
        partials rewritten and reduced."""
        torch = _torch()
        lib = _lib.load()
        m = int(chunk.size)
        if self._density_cols is None:
            self._density_cols = max(self.n_total - self.n_excluded_global(), 1)
        ops = self.gram_operand()
        self._sigma_pre = None  # (sums of the operand before these rows left it)
        if self.n:
            if int(self._density.shape[0]) < self.n_pad or not self._density.is_contiguous():
                raise ValueError("the cached density must hold one contiguous word per padded row")
            call("dal_density_downdate", _ptr(ops), self.n_pad, self.d_pad, _ptr(delta_ops), m,
                 _ptr(self._density), 0, _stream(self.device))
        _, loc = self._local_of(chunk)
        if loc.size:
            idx = torch.from_numpy(chunk).to(self.device)
            call("dal_mark_rows", _ptr(idx), m, self.row_base, self.n, DAL_ROW_EXCLUDED, _ptr(self.flags),
                 _stream(self.device))
            loc_t = torch.from_numpy(loc).to(self.device)
            for t in (ops, self._split_i8, self._split_fp4, self._u):
                if t is not None:
                    t.index_fill_(0, loc_t, 0)
            if self._colsum_partials is not None:
                touched = torch.from_numpy(np.unique(loc // DAL_CANON_CHUNK)).to(self.device)
                call("dal_canon_colsum_partials_chunks", _ptr(self.x), self.n, self.d, self.d, _ptr(self.norms()),
                     _ptr(self.flags), _ptr(touched), int(touched.shape[0]), _ptr(self._colsum_partials),
                     _stream(self.device))
                self._colsum = None if self._colsum is None else self.colsum(self._colsum_partials)
            else:
                self._colsum = None
        self._density_exact = None
        self._graphs = {}
        self._excluded_since_step = True
        self.excluded = np.union1d(self.excluded, chunk)
        self._downdate_err += float(lib.dal_density_downdate_error_bound(m, self.d_pad))

    def n_excluded_global(self) -> int:
        return int(self.excluded.size)

    def norms(self):
        """Canonical fp64 row norms [n]: those of the fused normalise+split
        pass once the Gram operand exists, else from dal_normalize_rows."""
        if self._norm64 is None:
            self.normalized()
        return self._norm64

    def normalized(self):
        """(u [n_pad, d_pad] fp32 with E rows zeroed, norm64 [n] fp64)."""
        if self._u is None:
            torch = _torch()
            if self.n == 0:
                self._u = torch.zeros((self.n_pad, self.d_pad), dtype=torch.float32, device=self.device)
                self._norm64 = torch.zeros(0, dtype=torch.float64, device=self.device)
                return self._u, self._norm64
            self._u = torch.empty((self.n_pad, self.d_pad), dtype=torch.float32, device=self.device)
            self._norm64 = torch.empty(self.n, dtype=torch.float64, device=self.device)
            call("dal_normalize_rows", _ptr(self.x), self.n, self.d, self.d, _ptr(self.flags),
                 self.n_pad, self.d_pad, _ptr(self._u), _ptr(self._norm64), _ptr(self.status),
                 _stream(self.device))
        return self._u, self._norm64

    def gram_operand(self, with_partials: bool = True, acc_zero=None):
        """The density GEMM's operand for this shard's rows: the fp32 unit rows
        (gram "f32") or their two-term fp16 split [n_pad, 2*d_pad] (gram
        "sym", dal_prep_split).  All-gathered as is in the multi-GPU path.
        with_partials: the fused prep also writes the canonical column-sum
        partials (else they are left to colsum_partials()).  acc_zero: an
        int64 [n_pad] density accumulator to zero (by the prep kernel when it
        runs here, else by a fill).  With ``prep_fused`` the same pass also
        writes the fp4 codes and the residual's sigma sums (dal_prep_split_fp4)."""
        if self.gram == "f32":
            u, _ = self.normalized()
            if acc_zero is not None:
                acc_zero.zero_()
            return u
        zeroed = False
        if self._split is None:
            torch = _torch()
            self._split = torch.empty((self.n_pad, 2 * self.d_pad), dtype=torch.int16, device=self.device)
            if self._u is not None:
                call("dal_split_f16", _ptr(self._u), self.n_pad, self.d_pad, self.d_pad, _ptr(self._split),
                     _stream(self.device))
            elif self.n == 0:  # an empty shard (more GPUs than row granules)
                self._split.zero_()
                if self._norm64 is None:
                    self._norm64 = torch.zeros(0, dtype=torch.float64, device=self.device)
            else:  # fused: the fp32 unit rows never reach HBM; canonical partials on the way
                norm64 = torch.empty(self.n, dtype=torch.float64, device=self.device)
                chunks = (self.n + DAL_CANON_CHUNK - 1) // DAL_CANON_CHUNK
                parts = None
                if self._colsum_partials is None and with_partials:
                    parts = torch.empty((chunks, self.d), dtype=torch.float64, device=self.device)
                if self.prep_fused and self._split_fp4 is None:
                    # one pass: the codes and the residual's sigma sums as well
                    self._split_fp4 = torch.empty((self.n_pad, self.d_pad // 2), dtype=torch.uint8,
                                                  device=self.device)
                    sig = torch.empty((self.n_pad // 512, self.d_pad), dtype=torch.int64, device=self.device)
                    s_l = torch.empty(self.d_pad, dtype=torch.int64, device=self.device)
                    wsb = int(_lib.load().dal_prep_split_fp4_workspace_bytes(self.n_pad, self.d_pad))
                    ws, wsp = workspace(wsb, self.device)
                    call("dal_prep_split_fp4", _ptr(self.x), self.n, self.d, self.d, _ptr(self.flags),
                         self.n_pad, self.d_pad, _ptr(self._split), _ptr(norm64),
                         0 if parts is None else _ptr(parts), 0 if acc_zero is None else _ptr(acc_zero),
                         _ptr(self._split_fp4), _ptr(sig), _ptr(s_l), wsp, wsb, _ptr(self.status),
                         _stream(self.device))
                    del ws
                    self._sigma_pre = (sig, s_l)
                else:
                    call("dal_prep_split", _ptr(self.x), self.n, self.d, self.d, _ptr(self.flags),
                         self.n_pad, self.d_pad, _ptr(self._split), _ptr(norm64),
                         0 if parts is None else _ptr(parts), 0 if acc_zero is None else _ptr(acc_zero),
                         _ptr(self.status), _stream(self.device))
                zeroed = True
                if self._norm64 is None:
                    self._norm64 = norm64
                if parts is not None:
                    self._colsum_partials = parts
        if acc_zero is not None and not zeroed:
            acc_zero.zero_()
        return self._split

    def gram_operand_i8(self, ops=None, n_rows=None):
        """The int8 form's MFMA operand a(H) [rows, d_pad] of the first
        ``n_rows`` rows of the split operand ``ops`` (dal_quant_i8).  This
        shard's own operand (the default) is quantised once and kept with the
        pool's caches; any other -- a gathered operand or a slice -- per call."""
        torch = _torch()
        own = self.gram_operand()
        if ops is None or ops is own or _ptr(ops) == _ptr(own):  # (a row prefix of the own operand included)
            if self._split_i8 is None:
                self._split_i8 = torch.empty((self.n_pad, self.d_pad), dtype=torch.int8, device=self.device)
                call("dal_quant_i8", _ptr(own), self.n_pad, self.d_pad, _ptr(self._split_i8), _stream(self.device))
            return self._split_i8
        n_rows = int(ops.shape[0]) if n_rows is None else int(n_rows)
        q = torch.empty((n_rows, self.d_pad), dtype=torch.int8, device=self.device)
        call("dal_quant_i8", _ptr(ops), n_rows, self.d_pad, _ptr(q), _stream(self.device))
        return q

    def gram_operand_fp4(self, ops=None, n_rows=None):
        """The fp4 form's MFMA operand, the e2m1 codes of a4(H) [rows, d_pad / 2]
        bytes (feature f in byte f / 2, the even one in the low nibble), of the
        first ``n_rows`` rows of the split operand ``ops`` (dal_quant_fp4).
        Cached and per call as gram_operand_i8."""
        torch = _torch()
        own = self.gram_operand()
        if ops is None or ops is own or _ptr(ops) == _ptr(own):  # (a row prefix of the own operand included)
            if self._split_fp4 is None:
                self._split_fp4 = torch.empty((self.n_pad, self.d_pad // 2), dtype=torch.uint8, device=self.device)
                call("dal_quant_fp4", _ptr(own), self.n_pad, self.d_pad, _ptr(self._split_fp4), _stream(self.device))
            return self._split_fp4
        n_rows = int(ops.shape[0]) if n_rows is None else int(n_rows)
        q = torch.empty((n_rows, self.d_pad // 2), dtype=torch.uint8, device=self.device)
        call("dal_quant_fp4", _ptr(ops), n_rows, self.d_pad, _ptr(q), _stream(self.device))
        return q

    def colsum_partials(self):
        """Canonical fp64 column-sum partials of this shard ([chunks, d])."""
        if self._colsum_partials is None:
            torch = _torch()
            norm64 = self.norms()
            chunks = (self.n + DAL_CANON_CHUNK - 1) // DAL_CANON_CHUNK
            self._colsum_partials = torch.empty((chunks, self.d), dtype=torch.float64, device=self.device)
            call("dal_canon_colsum_partials", _ptr(self.x), self.n, self.d, self.d, _ptr(norm64),
                 _ptr(self.flags), _ptr(self._colsum_partials), _stream(self.device))
        return self._colsum_partials

    def colsum(self, partials=None):
        """s = sum_{j not in E} u_j in the canonical fp64 order."""
        if partials is not None:
            torch = _torch()
            s = torch.empty(self.d, dtype=torch.float64, device=self.device)
            call("dal_canon_colsum_reduce", _ptr(partials), int(partials.shape[0]), self.d, _ptr(s),
                 _stream(self.device))
            return s
        if self._colsum is None:
            self._colsum = self.colsum(self.colsum_partials())
        return self._colsum

    def density_fixed(self, u_cols=None, n_cols_pad=None):
        """int64 fixed-point Gram row-sums (value * 2^32) of this shard's rows
        against every column of ``u_cols`` (default: this pool)."""
        if self._density is None or u_cols is not None:
            torch = _torch()
            op = self.gram_operand()
            if self.gram == "sym" and u_cols is not None:
                raise ValueError("gram 'sym' over a gathered operand: use ShardedSelector")
            if self.gram == "sym" and (self.row_base or self.n_total != self.n):
                raise ValueError("gram 'sym' on a shard: use ShardedSelector")
            if u_cols is None and self._acc_pre is not None:
                acc, self._acc_pre = self._acc_pre, None  # zeroed by the prep kernel
            else:
                acc = torch.zeros(self.n_pad, dtype=torch.int64, device=self.device)
            cols = op if u_cols is None else u_cols
            ncp = self.n_pad if n_cols_pad is None else int(n_cols_pad)
            self.gram_accumulate(acc, cols, ncp)
            if self.gram == "sym":
                self.gram_residual(acc, op)
            if u_cols is not None:
                return acc
            self.set_density_fixed(acc)
        return self._density

    def nb_active(self) -> int:
        """Global count of 256-row blocks (pad512(N_total) / 256)."""
        return (self.n_total + 511) // 512 * 2

    def gram_accumulate(self, acc, cols, n_cols_pad: int, grid_blocks: int = 0, col_row0: int = 0,
                        skip=None):
        """acc += fixed-point row sums of this shard's rows against the first
        ``n_cols_pad`` (a multiple of 512) rows of ``cols`` (a Gram operand of
        the pool's kind), whose first row is global row ``col_row0``.  Exact:
        any column split adds up to the same bits.

        gram "sym": acc is indexed by GLOBAL row (length >= nb_active * 256)
        and receives ONLY the row sums of this shard's own rows over the
        super-block pairs they take; the column sums of every pair come in
        closed form from gram_residual, so no collective follows (ABI v8).
        ``skip`` = (row0, row1), global column rows (multiples of 256) left
        out (gram "sym" only: already accumulated)."""
        torch = _torch()
        op = self.gram_operand()
        ev = None
        if self.gram_events is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        if self.gram == "sym":
            nb = self.nb_active()
            j_lo = col_row0 // 256
            j_hi = min(j_lo + int(n_cols_pad) // 256, nb)
            s_lo, s_hi = (0, 0) if skip is None else (skip[0] // 256, skip[1] // 256)
            if j_hi > j_lo and self.row_base // 256 < nb and self.gram_fp4:
                cols_fp4 = self.gram_operand_fp4(cols, (j_hi - j_lo) * 256)
                call("dal_gram_rowsum_sym_fp4_skip", _ptr(self.gram_operand_fp4()), self.row_base // 256,
                     self.n_pad // 256, _ptr(cols_fp4), j_lo, j_lo, j_hi, s_lo, s_hi, nb, self.d_pad, _ptr(acc),
                     int(grid_blocks), _stream(self.device))
            elif j_hi > j_lo and self.row_base // 256 < nb and self.gram_i8:
                cols_i8 = self.gram_operand_i8(cols, (j_hi - j_lo) * 256)
                call("dal_gram_rowsum_sym_i8_skip", _ptr(self.gram_operand_i8()), self.row_base // 256,
                     self.n_pad // 256, _ptr(cols_i8), j_lo, j_lo, j_hi, s_lo, s_hi, nb, self.d_pad, _ptr(acc),
                     int(grid_blocks), _stream(self.device))
            elif j_hi > j_lo and self.row_base // 256 < nb:
                call("dal_gram_rowsum_sym_skip", _ptr(op), self.row_base // 256, self.n_pad // 256,
                     _ptr(cols), j_lo, j_lo, j_hi, s_lo, s_hi, nb, self.d_pad, _ptr(acc), int(grid_blocks),
                     _stream(self.device))
        elif skip is not None:
            raise ValueError("a skipped column range needs gram 'sym'")
        else:
            call("dal_gram_rowsum", _ptr(op), self.n_pad, _ptr(cols), int(n_cols_pad), self.d_pad,
                 self.d_pad, _ptr(acc), int(grid_blocks), _stream(self.device))
        if ev is not None:
            ev[1].record()
            self.gram_events.append(ev)
        return acc

    def gram_residual(self, acc, ops):
        """Complete the compensated symmetric Gram (gram "sym"): add the exact
        remainder of the H-only A side for this shard's rows into acc (global
        row index).  ``ops``: the operand of EVERY active row (this pool's, or
        the gathered one on several GPUs)."""
        torch = _torch()
        lib = _lib.load()
        nb = self.nb_active()
        rb0, nrb = self.row_base // 256, self.n_pad // 256
        if rb0 >= nb or self.n == 0:
            return acc
        wsb = int(lib.dal_gram_sym_residual_workspace_bytes(nb, nrb, self.d_pad))
        ws, wsp = workspace(wsb, self.device)
        ev = None
        if self.gram_events is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        pre, self._sigma_pre = self._sigma_pre, None  # the fused prep's sums serve one residual
        if pre is not None and self.gram_fp4 and ops is self._split:
            call("dal_gram_sym_residual_fp4_pre", _ptr(ops), nb, rb0, nrb, self.d_pad, _ptr(acc), _ptr(pre[0]),
                 _ptr(pre[1]), wsp, wsb, _stream(self.device))
        else:
            name = ("dal_gram_sym_residual_fp4" if self.gram_fp4 else
                    "dal_gram_sym_residual_i8" if self.gram_i8 else "dal_gram_sym_residual")
            call(name, _ptr(ops), nb, rb0, nrb, self.d_pad, _ptr(acc), wsp, wsb, _stream(self.device))
        if ev is not None:
            ev[1].record()
            self.residual_events.append(ev)
        del ws
        return acc

    def events_off(self) -> bool:
        """No per-launch HIP-event timing requested (the graph path has none)."""
        return self.forest_events is None and self.select_events is None and self.gram_events is None

    def set_density_fixed(self, acc):
        """A cold Gram density of the current E (this pool's, or a shard's slice)."""
        self._density = acc
        self._density_cols, self._downdate_err = None, 0.0

    def density_exact(self, colsum=None):
        """Separable canonical fp64 density of this shard's rows (NaN for E):
        the exact identity sum_j <u_i,u_j> = <u_i, s>, O(N*D), bit-identical to
        the oracle.  ``colsum`` = the global s (multi-GPU); default this pool's."""
        if self._density_exact is None or colsum is not None:
            torch = _torch()
            norm64 = self.norms()
            s = self.colsum() if colsum is None else colsum
            d = torch.empty(self.n, dtype=torch.float64, device=self.device)
            call("dal_density_separable", _ptr(self.x), self.n, self.d, self.d, _ptr(norm64), _ptr(s),
                 _ptr(self.flags), _ptr(d), _stream(self.device))
            if colsum is not None:
                return d
            self._density_exact = d
        return self._density_exact

    def density(self, mode: str = "gram"):
        """fp64 density d[n] (NaN for rows in E): the MFMA Gram row-sum / 2^32
        (mode "gram", the reference's algorithm) or the exact separable form
        (mode "separable")."""
        torch = _torch()
        if mode == "separable":
            return self.density_exact()
        if mode != "gram":
            raise ValueError(f"density mode must be 'gram' or 'separable', not {mode!r}")
        d = self.density_fixed()[: self.n].to(torch.float64) * (1.0 / DAL_FIXED_SCALE)
        ex = (self.flags & DAL_ROW_EXCLUDED).bool()
        return torch.where(ex, torch.full_like(d, float("nan")), d)

    # ------------------------------------------------------------ helpers
    def row_flags(self, unlabeled_idx):
        """EXCLUDED bits | CANDIDATE for the (global) unlabeled indices of this
        shard, built on the device (no host round trip).  Returns (flags,
        unlabeled indices, count of unlabeled indices)."""
        unl = _as_index(unlabeled_idx, self.device)
        flags = self.flags.clone()
        call("dal_mark_rows", _ptr(unl), int(unl.shape[0]), self.row_base, self.n,
             DAL_ROW_CANDIDATE, _ptr(flags), _stream(self.device))
        return flags, unl, int(unl.shape[0])

    def local_positions(self, unl):
        """Rows of this shard for global indices ``unl`` (single GPU: all of them)."""
        if self.row_base == 0 and self.n == self.n_total:
            return unl
        loc = unl - self.row_base
        return loc[(loc >= 0) & (loc < self.n)]

    def check_status(self, st=None):
        """Raise on the device status word (``st``: a value already read)."""
        if st is None:
            st = int(self.status.item())
        if st & DAL_FLAG_ZERO_NORM:
            raise ValueError("pool contains a zero-norm row: cosine similarity is undefined "
                             "(the reference would propagate NaN into every density)")
        if st & DAL_FLAG_CAND_OVERFLOW:
            raise _lib.DalError("density re-rank candidate set exceeded DAL_SORT_CAP_PAYLOAD")
        if st & DAL_FLAG_SAMPLE_MISS:
            raise _lib.DalError("fast top-k level 1 overflowed and was not re-run")


GRAM_KINDS = ("sym", "f32")
GRAM_I8_MIN_BYTES = 32 << 20  # split operands above the contiguous schedule's limit take the int8 form
# 256-row chunks from which the fp4 form's one-pass preparation runs by default
# (PoolState(prep_fused=None)): its blocks own whole 512-row super blocks, so a
# small pool leaves most of the chip idle
PREP_FUSED_MIN_CHUNKS = 512


def _gram_kind(gram) -> str:
    """Density GEMM kernel: "sym" (default; fp16 MFMA on the two-term split,
    each symmetric block pair once, H-only taker side + exact closed-form
    remainder) or "f32" (fp32 MFMA on the unit rows, every pair: the
    plain-precision reference kernel, chosen per pool by the caller).  Both
    are within their rigorous bound of the canonical density and give the
    same (bit-exact) selection."""
    g = "sym" if gram is None else gram
    if g not in GRAM_KINDS:
        raise ValueError(f"gram must be one of {GRAM_KINDS}, not {g!r}")
    return g


def gram_products(state: PoolState) -> int:
    """fp16 MFMA products per feature pair of the pool's Gram kernel (bench
    roofline: executed vs algorithmic flops)."""
    return 1  # "sym": H.H alone since the H.L terms moved to the closed-form residual


def _as_index(idx, device):
    torch = _torch()
    if isinstance(idx, torch.Tensor):
        if idx.dtype is torch.int64 and idx.is_cuda and idx.get_device() == device.index and idx.is_contiguous():
            return idx  # already a device index list (the AL loop's steady state)
        return idx.to(device=device, dtype=torch.int64).contiguous()
    return torch.from_numpy(np.asarray(idx, dtype=np.int64).reshape(-1)).to(device)


def as_pool_state(pool, excluded=None, device=None) -> PoolState:
    if isinstance(pool, PoolState):
        if excluded is not None:
            pool.set_excluded(excluded)
        return pool
    return PoolState(pool, excluded=excluded, device=device)


_LUT_CACHE = {}


_SIDE_STREAMS = {}


def _side_stream(device):
    """One auxiliary HIP stream per device (created once)."""
    torch = _torch()
    key = str(device)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


def device_lut(strategy: str, n_trees: int, device):
    """fp64 LUT on the device, uploaded once per (strategy, T, device)."""
    torch = _torch()
    key = (strategy, int(n_trees), str(device))
    if key not in _LUT_CACHE:
        _LUT_CACHE[key] = torch.from_numpy(make_lut(strategy, n_trees)).to(device)
    return _LUT_CACHE[key]


def forest_score(state: PoolState, forest: Forest, lut_dev, flags, order: int, density=None,
                 density_err: float = 0.0, beta: float = 1.0, want_hi: bool = False,
                 density_kind=None, xb=None):
    """Launch dal_forest_score (dal_forest_score_blocked over ``xb``, the
    pool's blocked copy) over the shard; returns (votes, scores, keys, keys_hi)."""
    torch = _torch()
    forest.check_features(state.d)
    inner, leaf = forest.device(state.device)
    n = state.n
    votes = torch.empty(n, dtype=torch.int32, device=state.device)
    scores = torch.empty(n, dtype=torch.float64, device=state.device)
    keys = torch.empty(n, dtype=torch.int64, device=state.device)
    keys_hi = torch.empty(n, dtype=torch.int64, device=state.device) if want_hi else None
    if density is None:
        kind = DAL_DENSITY_NONE
    elif density_kind is not None:
        kind = density_kind
    else:
        kind = DAL_DENSITY_EXACT if density.dtype == torch.float64 else DAL_DENSITY_FIXED
    ev = None
    if state.forest_events is not None:  # bench: K2 launch timing on the launch stream
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        if state.event_lead_cycles:
            torch.cuda._sleep(state.event_lead_cycles)
        ev[0].record()
    args = (n, state.d, state.d, _ptr(inner), _ptr(leaf), forest.n_trees, forest.depth, _ptr(lut_dev),
            0 if density is None else _ptr(density), kind, float(density_err), _ptr(flags), float(beta), int(order),
            _ptr(votes), _ptr(scores), _ptr(keys), 0 if keys_hi is None else _ptr(keys_hi), _stream(state.device))
    for _ in range(state.event_repeat if ev is not None else 1):
        if xb is None:
            call("dal_forest_score", _ptr(state.x), *args)
        else:
            call("dal_forest_score_blocked", _ptr(state.x), _ptr(xb), _fprep(forest, state, xb), *args)
    if ev is not None:
        ev[1].record()
        state.forest_events.append(ev)
    return votes, scores, keys, keys_hi


MULTICLASS_KINDS = {"least_confidence": DAL_MC_LEAST_CONFIDENCE, "margin": DAL_MC_MARGIN,
                    "entropy": DAL_MC_ENTROPY}


def device_multiclass_lut(strategy: str, n_trees: int, device):
    """The multiclass fp64 LUT on the device, uploaded once per (strategy, T, device)."""
    torch = _torch()
    key = ("multiclass", strategy, int(n_trees), str(device))
    if key not in _LUT_CACHE:
        _LUT_CACHE[key] = torch.from_numpy(multiclass_lut(strategy, n_trees)).to(device)
    return _LUT_CACHE[key]


def forest_score_multiclass(state: PoolState, forest: Forest, lut_dev, flags, order: int, kind: int, xb=None):
    """Launch dal_forest_score_multiclass (dal_forest_score_multiclass_blocked
    over ``xb``, the pool's blocked copy: same bits) over the shard; returns
    (counts uint8 [n, C], pred uint8 [n], scores, keys).  flags None: every
    row is a candidate."""
    torch = _torch()
    forest.check_features(state.d)
    forest.check_classes()
    if forest.n_trees > DAL_MC_MAX_TREES:
        raise ValueError(f"a multiclass forest may hold at most {DAL_MC_MAX_TREES} trees, not {forest.n_trees}")
    inner, leaf = forest.device(state.device)
    n, C = state.n, int(forest.n_classes)
    counts = torch.empty((n, C), dtype=torch.uint8, device=state.device)
    pred = torch.empty(n, dtype=torch.uint8, device=state.device)
    scores = torch.empty(n, dtype=torch.float64, device=state.device)
    keys = torch.empty(n, dtype=torch.int64, device=state.device)
    args = (n, state.d, state.d, _ptr(inner), _ptr(leaf), forest.n_trees, forest.depth, C, _ptr(lut_dev), int(kind),
            0 if flags is None else _ptr(flags), int(order), _ptr(counts), _ptr(pred), _ptr(scores), _ptr(keys),
            _stream(state.device))
    if xb is None:
        call("dal_forest_score_multiclass", _ptr(state.x), *args)
    else:
        call("dal_forest_score_multiclass_blocked", _ptr(state.x), _ptr(xb), _fprep(forest, state, xb), *args)
    return counts, pred, scores, keys


def soft_proba(sums, denominator: int):
    """fp64 (double)S_c / (double)M of int64 class sums: one IEEE division per
    entry (a tensor divisor: dividing a device tensor by a Python float
    multiplies by its reciprocal)."""
    torch = _torch()
    p = sums.to(torch.float64)
    return p / p.new_full((1,), float(denominator))


SOFT_KINDS = {"least_confidence": _lib.DAL_SOFT_LEAST_CONFIDENCE, "margin": _lib.DAL_SOFT_MARGIN,
              "entropy": _lib.DAL_SOFT_ENTROPY}


def forest_score_soft(state: PoolState, forest, flags, order: int, kind: int):
    """Launch dal_forest_score_soft over the shard: the exact class sums of a
    ProbabilityForest's leaf distributions and the soft-vote score; returns
    (sums int64 [n, C], pred uint8 [n], scores, keys).  flags None: every row
    is a candidate."""
    torch = _torch()
    forest.check_features(state.d)
    inner, leaf_id, leaf_q = forest.device(state.device)  # (checks the limits and the leaf ids before the upload)
    n, C = state.n, int(forest.n_classes)
    sums = torch.empty((n, C), dtype=torch.int64, device=state.device)
    pred = torch.empty(n, dtype=torch.uint8, device=state.device)
    scores = torch.empty(n, dtype=torch.float64, device=state.device)
    keys = torch.empty(n, dtype=torch.int64, device=state.device)
    call("dal_forest_score_soft", _ptr(state.x), n, state.d, state.d, _ptr(inner), _ptr(leaf_id), _ptr(leaf_q),
         forest.n_leaves, forest.n_trees, int(forest.depth), C, int(kind), 0 if flags is None else _ptr(flags),
         int(order), _ptr(sums), _ptr(pred), _ptr(scores), _ptr(keys), _stream(state.device))
    return sums, pred, scores, keys


def forest_score_soft_bald(state: PoolState, forest, flags, order: int = DAL_DESCENDING):
    """Launch dal_forest_score_soft_bald over the shard: the trees'
    disagreement H(pbar) - (1/T) sum_t H(p_t) of a ProbabilityForest (BALD, the
    mean KL divergence to the consensus), on the forest's own leaf entropy
    words (``forest.leaf_h``).  Returns (sums int64 [n, C], pred uint8 [n],
    hsum int64 [n], entropy fp64 [n] -- dal_forest_score_soft's entropy, the
    same bits --, scores, keys).  flags None: every row is a candidate."""
    torch = _torch()
    forest.check_features(state.d)
    inner, leaf_id, leaf_q = forest.device(state.device)  # (checks the limits and the leaf ids before the upload)
    leaf_h = forest.device_leaf_h(state.device)
    dev = state.device
    n, C = state.n, int(forest.n_classes)
    sums = torch.empty((n, C), dtype=torch.int64, device=dev)
    pred = torch.empty(n, dtype=torch.uint8, device=dev)
    hsum = torch.empty(n, dtype=torch.int64, device=dev)
    entropy = torch.empty(n, dtype=torch.float64, device=dev)
    scores = torch.empty(n, dtype=torch.float64, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    call("dal_forest_score_soft_bald", _ptr(state.x), n, state.d, state.d, _ptr(inner), _ptr(leaf_id), _ptr(leaf_q),
         _ptr(leaf_h), forest.n_leaves, forest.n_trees, int(forest.depth), C, 0 if flags is None else _ptr(flags),
         int(order), _ptr(sums), _ptr(pred), _ptr(hsum), _ptr(entropy), _ptr(scores), _ptr(keys), _stream(dev))
    return sums, pred, hsum, entropy, scores, keys


def forest_score_soft_dw(state: PoolState, forest, flags, density, density_kind: int, density_err: float = 0.0,
                         beta: float = 1.0, want_hi: bool = True):
    """Launch dal_forest_score_soft_dw over the shard: the soft-vote class
    entropy (dal_forest_score_soft's, the same bits) x density^beta,
    descending, with interval keys.  ``density``: one 8-byte word per row,
    int64 fixed point (DAL_DENSITY_FIXED) or canonical fp64
    (DAL_DENSITY_EXACT).  Returns (sums int64 [n, C], pred uint8 [n], entropy
    fp64 [n], row_index int32 [n], scores, keys, keys_hi or None).  flags
    None: every row is a candidate."""
    torch = _torch()
    forest.check_features(state.d)
    if density_kind not in (DAL_DENSITY_FIXED, DAL_DENSITY_EXACT):
        raise ValueError("density_kind must be DAL_DENSITY_FIXED or DAL_DENSITY_EXACT")
    if density is None or int(density.shape[0]) < state.n or density.element_size() != 8:
        raise ValueError("density must hold one 8-byte word per row of the pool")
    inner, leaf_id, leaf_q = forest.device(state.device)  # (checks the limits and the leaf ids before the upload)
    dev = state.device
    n, C = state.n, int(forest.n_classes)
    sums = torch.empty((n, C), dtype=torch.int64, device=dev)
    pred = torch.empty(n, dtype=torch.uint8, device=dev)
    entropy = torch.empty(n, dtype=torch.float64, device=dev)
    row_index = torch.empty(n, dtype=torch.int32, device=dev)
    scores = torch.empty(n, dtype=torch.float64, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    keys_hi = torch.empty(n, dtype=torch.int64, device=dev) if want_hi else None
    ev = None
    if state.forest_events is not None:  # bench: K2 launch timing on the launch stream
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    call("dal_forest_score_soft_dw", _ptr(state.x), n, state.d, state.d, _ptr(inner), _ptr(leaf_id), _ptr(leaf_q),
         forest.n_leaves, forest.n_trees, int(forest.depth), C, _ptr(density), int(density_kind), float(density_err),
         0 if flags is None else _ptr(flags), float(beta), _ptr(sums), _ptr(pred), _ptr(entropy), _ptr(row_index),
         _ptr(scores), _ptr(keys), 0 if keys_hi is None else _ptr(keys_hi), _stream(dev))
    if ev is not None:
        ev[1].record()
        state.forest_events.append(ev)
    return sums, pred, entropy, row_index, scores, keys, keys_hi


def forest_score_multiclass_dw(state: PoolState, forest: Forest, flags, density, density_kind: int,
                               density_err: float = 0.0, beta: float = 1.0, want_hi: bool = True, xb=None):
    """Launch dal_forest_score_multiclass_dw (dal_forest_score_multiclass_dw_
    blocked over ``xb``, the pool's blocked copy: same bits) over the shard:
    class entropy x density^beta, descending, with interval keys.  ``density``: one 8-byte
    word per row, int64 fixed point (DAL_DENSITY_FIXED) or canonical fp64
    (DAL_DENSITY_EXACT).  Returns (counts uint8 [n, C], pred uint8 [n],
    entropy fp64 [n], row_index int32 [n], scores, keys, keys_hi or None).
    flags None: every row is a candidate."""
    torch = _torch()
    forest.check_features(state.d)
    forest.check_classes()
    if forest.n_trees > DAL_MC_MAX_TREES:
        raise ValueError(f"a multiclass forest may hold at most {DAL_MC_MAX_TREES} trees, not {forest.n_trees}")
    if density_kind not in (DAL_DENSITY_FIXED, DAL_DENSITY_EXACT):
        raise ValueError("density_kind must be DAL_DENSITY_FIXED or DAL_DENSITY_EXACT")
    if density is None or int(density.shape[0]) < state.n or density.element_size() != 8:
        raise ValueError("density must hold one 8-byte word per row of the pool")
    inner, leaf = forest.device(state.device)
    dev = state.device
    n, C = state.n, int(forest.n_classes)
    lut_dev = device_multiclass_lut("entropy", forest.n_trees, dev)
    counts = torch.empty((n, C), dtype=torch.uint8, device=dev)
    pred = torch.empty(n, dtype=torch.uint8, device=dev)
    entropy = torch.empty(n, dtype=torch.float64, device=dev)
    row_index = torch.empty(n, dtype=torch.int32, device=dev)
    scores = torch.empty(n, dtype=torch.float64, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    keys_hi = torch.empty(n, dtype=torch.int64, device=dev) if want_hi else None
    ev = None
    if state.forest_events is not None:  # bench: K2 launch timing on the launch stream
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    args = (n, state.d, state.d, _ptr(inner), _ptr(leaf), forest.n_trees, forest.depth, C, _ptr(lut_dev),
            _ptr(density), int(density_kind), float(density_err), 0 if flags is None else _ptr(flags), float(beta),
            _ptr(counts), _ptr(pred), _ptr(entropy), _ptr(row_index), _ptr(scores), _ptr(keys),
            0 if keys_hi is None else _ptr(keys_hi), _stream(dev))
    if xb is None:
        call("dal_forest_score_multiclass_dw", _ptr(state.x), *args)
    else:
        call("dal_forest_score_multiclass_dw_blocked", _ptr(state.x), _ptr(xb), _fprep(forest, state, xb), *args)
    if ev is not None:
        ev[1].record()
        state.forest_events.append(ev)
    return counts, pred, entropy, row_index, scores, keys, keys_hi


def _fprep(forest: Forest, state: PoolState, xb) -> int:
    """Address of the forest prepared for the blocked kernel (0 without xb)."""
    if xb is None:
        return 0
    p = forest.blocked_prep(state.device, state.d)
    return 0 if p is None else _ptr(p)


def topk_keys(keys, k: int, idx_base: int = 0):
    """k smallest keys (ties -> lower index): (indices int64 [k], keys [k])."""
    torch = _torch()
    lib = _lib.load()
    n = int(keys.shape[0])
    ws = torch.empty(int(lib.dal_topk_workspace_bytes(n, k)) + 256, dtype=torch.uint8,
                     device=keys.device)
    wsp = (_ptr(ws) + 255) // 256 * 256
    out_idx = torch.empty(k, dtype=torch.int64, device=keys.device)
    out_keys = torch.empty(k, dtype=torch.int64, device=keys.device)
    call("dal_topk", _ptr(keys), n, k, int(idx_base), wsp, int(lib.dal_topk_workspace_bytes(n, k)),
         _ptr(out_idx), _ptr(out_keys), _stream(keys.device))
    return out_idx, out_keys


def density_error(state: PoolState) -> float:
    """Bound on |d_gemm - d_canonical| (rigorous; dal_density_error_bound or
    _sym, by the pool's Gram kernel; after PoolState.exclude the cached
    density's cold bound plus dal_density_downdate_error_bound per downdate)."""
    n_cols = max(state.n_total - state.n_excluded_global(), 1)
    lib = _lib.load()
    if state.gram == "f32":
        return float(lib.dal_density_error_bound(n_cols))
    if state._density_cols is not None:
        # after PoolState.exclude: the cold Gram's bound at the columns it
        # summed, plus the bounds of the downdates applied since
        return float(lib.dal_density_error_bound_sym_d(state._density_cols, state.d_pad)) + state._downdate_err
    return float(lib.dal_density_error_bound_sym_d(n_cols, state.d_pad))


def candidate_cap(n: int, k: int) -> int:
    """Initial re-rank candidate capacity (grown on overflow).  Up to
    DAL_SORT_CAP_PAYLOAD the exact second level is a single one-block sort."""
    return int(min(n, max(4 * k, _lib.DAL_SORT_CAP_PAYLOAD)))


# Fast level 1 of the interval selections (ABI v6): tau = the k-th smallest
# of <= 4096 row groups' minimum keys bounds the candidate search (group
# minima + one launch instead of 6 radix passes + 3 compaction launches);
# 0 selects the exact radix level 1 (after an overflow, per pool).
LEVEL1_PASSES = 1


def level1_passes(state, n: int, k: int, cap: int) -> int:
    if not state.level1_fast or cap > DAL_SORT_CAP_PAYLOAD:
        return 0
    return LEVEL1_PASSES


def workspace(nbytes: int, device):
    """A 256-byte aligned device workspace: (tensor, aligned pointer)."""
    torch = _torch()
    ws = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
    return ws, (_ptr(ws) + 255) // 256 * 256


def dw_select_local(state: PoolState, flags, votes, keys_lo, keys_hi, lut_dev, k: int,
                    beta: float, colsum, cap_scale: int = 1, sync: bool = True, colsum_ready=None):
    """dal_dw_select on this shard: exact canonical top-k of the shard.  The
    candidate capacity grows (and the step re-runs) on DAL_FLAG_CAND_OVERFLOW.
    colsum_ready: a torch.cuda.Event recorded after ``colsum`` on another
    stream; the library joins it just before the re-rank (its only reader).
    sync=False: no status read here -- the caller checks state.status later
    and re-runs with a larger cap_scale on overflow (multi-GPU path)."""
    torch = _torch()
    lib = _lib.load()
    n = state.n
    norm64 = state.norms()
    if sync:  # single-GPU: start from the capacity a previous overflow grew to
        cap_scale = max(cap_scale, state.cap_scale)
    base = candidate_cap(n, k) if state.cap_base is None else max(int(k), int(state.cap_base))
    cap = int(min(n, base * cap_scale))
    while True:
        passes = level1_passes(state, n, k, cap)
        wsb = int(lib.dal_dw_select_workspace_bytes(n, k, cap))
        ws, wsp = workspace(wsb, state.device)
        out_idx = torch.empty(k, dtype=torch.int64, device=state.device)
        out_scores = torch.empty(k, dtype=torch.float64, device=state.device)
        out_keys = torch.empty(k, dtype=torch.int64, device=state.device)
        ev = None
        if state.select_events is not None:  # bench: K3 timing on the launch stream
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            if state.event_lead_cycles:
                torch.cuda._sleep(state.event_lead_cycles)
            ev[0].record()
        for _ in range(state.event_repeat if ev is not None else 1):
            call("dal_dw_select", _ptr(keys_lo), _ptr(keys_hi), _ptr(votes), _ptr(flags), n, k,
                 state.row_base, _ptr(lut_dev), float(beta), _ptr(state.x), state.d, state.d,
                 _ptr(norm64), _ptr(colsum), cap, passes, wsp, wsb, _ptr(out_idx), _ptr(out_scores),
                 _ptr(out_keys), _ptr(state.status),
                 0 if colsum_ready is None else colsum_ready.cuda_event, _stream(state.device))
        if ev is not None:
            ev[1].record()
            state.select_events.append(ev)
        if not sync:
            return out_idx, out_scores, out_keys
        # the step's one host sync: status word (zero-norm rows, candidate overflow)
        st = int(state.status.item())
        state.last_status = st
        if st & DAL_FLAG_SAMPLE_MISS:  # fast level 1 over capacity: exact level 1 from now on
            state.status.bitwise_and_(~(DAL_FLAG_SAMPLE_MISS | DAL_FLAG_CAND_OVERFLOW))
            state.level1_fast = False
            continue
        if cap >= n or not (st & DAL_FLAG_CAND_OVERFLOW):
            return out_idx, out_scores, out_keys
        state.status.bitwise_and_(~DAL_FLAG_CAND_OVERFLOW)
        cap = min(n, cap * 4)
        state.cap_scale *= 4  # later steps (same pool, same score spread) start here


def dw_step_local(state: PoolState, forest: Forest, flags, dens, lut_dev, k: int, beta: float, colsum,
                  colsum_ready=None, cap_scale: int = None, sync: bool = True, xb=None, n_classes=None,
                  soft: bool = False):
    """dal_dw_step on this pool or shard: votes, scores and interval keys
    of every row, then the exact canonical top-k -- one C call with fused
    launches (the fast level 1; ``xb``: the pool's blocked copy for the score
    kernel).  Same retries as dw_select_local.
    ``n_classes`` (None: the binary step): dal_dw_step_multiclass over a
    C-class forest -- ``lut_dev`` is then the multiclass entropy table, ``xb``
    the copy the C-class rule allowed, and per-class counts ([n, C] uint8)
    come back in the place of the votes.
    ``soft``: dal_dw_step_soft over a ProbabilityForest on the row-major pool
    (``lut_dev``, ``xb`` and ``n_classes`` unused); the class sums ([n, C]
    int64) come back in the place of the votes.
    Returns (votes, scores, indices, selected scores); sync=False (the
    multi-GPU path: the caller reads the status word after the merge and
    re-runs with a larger ``cap_scale``) also returns the selected keys."""
    torch = _torch()
    lib = _lib.load()
    n = state.n
    forest.check_features(state.d)
    norm64 = state.norms()
    derr = float(density_error(state))
    dev = state.device
    if soft:
        inner, leaf_id, leaf_q = forest.device(dev)  # (checks the limits and the leaf ids before the upload)
        votes = torch.empty((n, int(forest.n_classes)), dtype=torch.int64, device=dev)  # the class sums
        entropy = torch.empty(n, dtype=torch.float64, device=dev)
        row_index = torch.empty(n, dtype=torch.int32, device=dev)
        entry, rows = "dal_dw_step_soft", (_ptr(votes), 0, _ptr(entropy), _ptr(row_index))
        head = (_ptr(state.x), n, state.d, state.d, _ptr(inner), _ptr(leaf_id), _ptr(leaf_q), forest.n_leaves,
                forest.n_trees, int(forest.depth), int(forest.n_classes))
    elif n_classes is None:
        inner, leaf = forest.device(dev)
        votes = torch.empty(n, dtype=torch.int32, device=dev)
        entry, classes, rows = "dal_dw_step", (), (_ptr(votes),)
    else:
        inner, leaf = forest.device(dev)
        forest.check_classes()
        if forest.n_trees > DAL_MC_MAX_TREES:
            raise ValueError(f"a multiclass forest may hold at most {DAL_MC_MAX_TREES} trees, not {forest.n_trees}")
        votes = torch.empty((n, int(n_classes)), dtype=torch.uint8, device=dev)  # the per-class counts
        entropy = torch.empty(n, dtype=torch.float64, device=dev)
        row_index = torch.empty(n, dtype=torch.int32, device=dev)
        # (pred is not kept: a Selection carries the counts)
        entry, classes, rows = "dal_dw_step_multiclass", (int(n_classes),), (_ptr(votes), 0, _ptr(entropy),
                                                                              _ptr(row_index))
    scores = torch.empty(n, dtype=torch.float64, device=dev)
    keys_lo = torch.empty(n, dtype=torch.int64, device=dev)
    keys_hi = torch.empty(n, dtype=torch.int64, device=dev)
    base = candidate_cap(n, k) if state.cap_base is None else max(int(k), int(state.cap_base))
    cap = int(min(n, base * (state.cap_scale if cap_scale is None else cap_scale)))
    if not soft:
        head = (_ptr(state.x), 0 if xb is None else _ptr(xb), _fprep(forest, state, xb), n, state.d, state.d,
                _ptr(inner), _ptr(leaf), forest.n_trees, forest.depth, *classes, _ptr(lut_dev))
    while True:
        passes = level1_passes(state, n, k, cap)
        wsb = int(lib.dal_dw_step_workspace_bytes(n, k, cap))
        # one workspace per (n, k, cap), zeroed once: DAL_STEP_WS_CLEAN leaves
        # its header zero after every call (no zeroing launch per step)
        key = (n, k, cap)
        if key not in state._ws_clean:
            ws, wsp = workspace(wsb, dev)
            ws.zero_()
            state._ws_clean[key] = (ws, wsp)
        ws, wsp = state._ws_clean[key]
        out_idx = torch.empty(k, dtype=torch.int64, device=dev)
        out_scores = torch.empty(k, dtype=torch.float64, device=dev)
        out_keys = None if sync else torch.empty(k, dtype=torch.int64, device=dev)
        try:
            call(entry, *head, _ptr(dens), derr, _ptr(flags), float(beta), state.row_base,
                 _ptr(norm64), _ptr(colsum), k, cap, passes, DAL_STEP_WS_CLEAN, wsp, wsb, *rows,
                 _ptr(scores), _ptr(keys_lo), _ptr(keys_hi), _ptr(out_idx), _ptr(out_scores),
                 0 if out_keys is None else _ptr(out_keys), _ptr(state.status),
                 0 if colsum_ready is None else colsum_ready.cuda_event, _stream(dev))
        except _lib.DalError:
            # a call that failed after queueing part of the step may leave the
            # level-1 header dirty: never reuse this workspace as "clean"
            state._ws_clean.pop(key, None)
            raise
        if not sync:
            return votes, scores, out_idx, out_scores, out_keys
        st = int(state.status.item())  # the step's one host sync
        state.last_status = st
        if st & DAL_FLAG_SAMPLE_MISS:  # fast level 1 over capacity: exact level 1 from now on
            state.status.bitwise_and_(~(DAL_FLAG_SAMPLE_MISS | DAL_FLAG_CAND_OVERFLOW))
            state.level1_fast = False
            continue
        if cap >= n or not (st & DAL_FLAG_CAND_OVERFLOW):
            return votes, scores, out_idx, out_scores
        state.status.bitwise_and_(~DAL_FLAG_CAND_OVERFLOW)
        cap = min(n, cap * 4)
        state.cap_scale *= 4


def sort_pairs(keys, idx, k: int, payload=None):
    """Sort (key, idx) pairs (with an optional fp64 payload) and keep k."""
    torch = _torch()
    n = int(keys.shape[0])
    k = min(k, n)
    out_keys = torch.empty(k, dtype=torch.int64, device=keys.device)
    out_idx = torch.empty(k, dtype=torch.int64, device=keys.device)
    out_pay = torch.empty(k, dtype=torch.float64, device=keys.device) if payload is not None else None
    call("dal_sort_pairs", _ptr(keys), _ptr(idx), 0 if payload is None else _ptr(payload), n, k,
         _ptr(out_keys), _ptr(out_idx), 0 if out_pay is None else _ptr(out_pay), _stream(keys.device))
    return out_keys, out_idx, out_pay


# ---------------------------------------------------------------- steps --
def uncertainty_blocked(state: PoolState, forest: Forest, multiclass: bool = None):
    """The blocked pool copy for an uncertainty step (scores only, no
    density: every step is alike; ``multiclass`` as PoolState.blocked_pool):
    built from the pool's second step on --
    the one-off copy costs about five row-major score launches (2M x 256:
    0.92 ms vs 0.2 ms saved per launch), so a pool scored once keeps the
    row-major kernel."""
    state._us_steps += 1
    return state.blocked_pool(forest, build=state._us_steps > 1, multiclass=multiclass)


def uncertainty_step(state: PoolState, unlabeled_idx, forest: Forest, k: int,
                     strategy: str = "least_confidence") -> Selection:
    """One iteration of uncertainty_sampling.py:85-112 on the GPU."""
    flags, unl, n_cand = state.row_flags(unlabeled_idx)
    if n_cand == 0:
        raise ValueError("unlabeled set is empty (the reference loop breaks here)")
    kk = min(int(k), n_cand)
    loc = state.local_positions(unl)
    order = DAL_ASCENDING if ASCENDING[strategy] else DAL_DESCENDING
    lut_dev = device_lut(strategy, forest.n_trees, state.device)
    votes, scores, keys, _ = forest_score(state, forest, lut_dev, flags, order,
                                          xb=uncertainty_blocked(state, forest))
    idx, _ = topk_keys(keys, kk, state.row_base)
    sel_scores = scores[idx - state.row_base]
    state.check_status()
    return Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, votes=(votes, loc))


def multiclass_step(state: PoolState, unlabeled_idx, forest: Forest, k: int,
                    strategy: str = "least_confidence") -> Selection:
    """One uncertainty iteration over a C-class forest: per-class votes and
    the C-class score (dal_forest_score_multiclass; from the pool's second
    uncertainty step on over its blocked copy, the binary policy), then the
    top-k of the keys.  The Selection carries ``counts`` ([U, C] uint8); ``votes`` is None."""
    if strategy not in MULTICLASS_KINDS:
        raise ValueError(f"strategy must be one of {tuple(MULTICLASS_KINDS)}")
    flags, unl, n_cand = state.row_flags(unlabeled_idx)
    if n_cand == 0:
        raise ValueError("unlabeled set is empty (the reference loop breaks here)")
    kk = min(int(k), n_cand)
    loc = state.local_positions(unl)
    order = DAL_ASCENDING if MULTICLASS_ASCENDING[strategy] else DAL_DESCENDING
    lut_dev = device_multiclass_lut(strategy, forest.n_trees, state.device)
    counts, _, scores, keys = forest_score_multiclass(state, forest, lut_dev, flags, order,
                                                      MULTICLASS_KINDS[strategy],
                                                      xb=uncertainty_blocked(state, forest, multiclass=True))
    idx, _ = topk_keys(keys, kk, state.row_base)
    sel_scores = scores[idx - state.row_base]
    return Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, counts=(counts, loc))


def soft_step(state: PoolState, unlabeled_idx, forest, k: int, strategy: str = "least_confidence") -> Selection:
    """One uncertainty iteration over a ProbabilityForest: the averaged leaf
    class distributions and the soft-vote score (dal_forest_score_soft), then
    the top-k of the keys.  Scores, indices and selected scores as
    multiclass_step; the Selection carries ``sums`` ([U, C] int64) and
    ``proba()``; ``votes`` and ``counts`` are None.  strategy="bald": the
    trees' disagreement (dal_forest_score_soft_bald), descending; the
    Selection also carries ``entropy`` (fp64 [U]) and ``hsum`` (int64 [U])."""
    if strategy not in SOFT_KINDS and strategy != "bald":
        raise ValueError(f"strategy must be one of {tuple(SOFT_KINDS) + ('bald',)}")
    flags, unl, n_cand = state.row_flags(unlabeled_idx)
    if n_cand == 0:
        raise ValueError("unlabeled set is empty (the reference loop breaks here)")
    kk = min(int(k), n_cand)
    loc = state.local_positions(unl)
    entropy = hsum = None
    if strategy == "bald":
        sums, _, hsum, entropy, scores, keys = forest_score_soft_bald(state, forest, flags, DAL_DESCENDING)
        entropy, hsum = (entropy, loc), (hsum, loc)
    else:
        order = DAL_ASCENDING if MULTICLASS_ASCENDING[strategy] else DAL_DESCENDING
        sums, _, scores, keys = forest_score_soft(state, forest, flags, order, SOFT_KINDS[strategy])
    idx, _ = topk_keys(keys, kk, state.row_base)
    sel_scores = scores[idx - state.row_base]
    return Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, sums=(sums, loc),
                     denominator=forest.denominator, entropy=entropy, hsum=hsum)


def soft_density_step(state: PoolState, unlabeled_idx, forest, k: int, beta: float = 1.0, density_fixed=None,
                      mode: str = "gram") -> Selection:
    """One density-weighted iteration over a ProbabilityForest: score =
    entropy(predict_proba) x d^beta, descending; exact canonical selection on
    the entropy the kernel returned ("K2 soft votes,
    density-weighted").

    mode "gram": as multiclass_density_step -- on a cold pool the Gram goes
    first with the canonical column sum on the side stream, then one
    dal_dw_step_soft call (dw_step_local's clean workspace): interval keys,
    per-row entropy and the identity index, and the selection with lut =
    entropy, votes = row index, whose fp64 re-rank forms entropy[i] *
    (canonical density)^beta.  With ``forest_events`` or ``select_events`` set
    the unfused pair runs (dal_forest_score_soft_dw, dal_dw_select).  The
    soft kernel reads the row-major pool on every step: there is no blocked
    copy and no graph plan.
    mode "separable": the exact O(N*D) density, canonical scores for every
    row and a plain top-k.
    The Selection carries ``sums`` ([U, C] int64) and ``proba()``, as
    soft_step's."""
    if mode not in ("gram", "separable"):
        raise ValueError(f"density mode must be 'gram' or 'separable', not {mode!r}")
    unl = _as_index(unlabeled_idx, state.device)
    if int(unl.shape[0]) == 0:
        raise ValueError("unlabeled set is empty (the reference loop breaks here)")
    if mode == "separable":
        flags, unl, n_cand = state.row_flags(unl)
        kk = min(int(k), n_cand)
        loc = state.local_positions(unl)
        sums, _, _, _, scores, keys, _ = forest_score_soft_dw(
            state, forest, flags, state.density_exact(), DAL_DENSITY_EXACT, beta=beta, want_hi=False)
        idx, _ = topk_keys(keys, kk, state.row_base)
        sel_scores = scores[idx - state.row_base]
        state.check_status()
        return Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, sums=(sums, loc),
                         denominator=forest.denominator)
    state._excluded_since_step = False
    # the density GEMM goes to the GPU first; the host prepares the rest while it runs
    dens, colsum_ready = _density_for_step(state, density_fixed)
    flags, unl, n_cand = state.row_flags(unl)
    kk = min(int(k), n_cand)
    loc = state.local_positions(unl)
    if state.forest_events is None and state.select_events is None:
        sums, scores, idx, sel_scores = dw_step_local(state, forest, flags, dens, None, kk, beta, state.colsum(),
                                                      colsum_ready, soft=True)
    else:  # the per-kernel timing path keeps K2 / K3 apart
        sums, _, entropy, row_index, scores, keys_lo, keys_hi = forest_score_soft_dw(
            state, forest, flags, dens, DAL_DENSITY_FIXED, density_err=density_error(state), beta=beta, want_hi=True)
        # the main stream joins the column sum inside the call, just before the re-rank
        idx, sel_scores, _ = dw_select_local(state, flags, row_index, keys_lo, keys_hi, entropy, kk, beta,
                                             state.colsum(), colsum_ready=colsum_ready)
    state.check_status(state.last_status)  # the word the step read (no second sync)
    return Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, sums=(sums, loc),
                     denominator=forest.denominator)


def multiclass_density_step(state: PoolState, unlabeled_idx, forest: Forest, k: int, beta: float = 1.0,
                            density_fixed=None, mode: str = "gram") -> Selection:
    """One density-weighted iteration over a C-class forest (C >= 2): score =
    class entropy x d^beta, descending; exact canonical selection (DESIGN.md,
    "K2 multiclass, density-weighted").

    mode "gram": as density_step's unfused branch -- on a cold pool the Gram
    goes first with the canonical column sum on the side stream, then
    dal_forest_score_multiclass_dw (interval keys, per-row entropy and the
    identity index) and dal_dw_select with lut = entropy, votes = row index:
    its fp64 re-rank forms entropy[i] * (canonical density)^beta.  A warm
    step (the density cached or handed in) scores over the pool's blocked
    copy (dal_forest_score_multiclass_dw_blocked, same bits; density_step's
    rule), built by the first warm step.  As in density_step, a warm step on
    the whole pool replays a cached plan (WarmStepGraph with n_classes:
    dal_dw_plan_create_multiclass) when ``use_graphs`` is set and no events
    are requested; a cold step, a handed-in density or a shard is one
    dal_dw_step_multiclass call (dw_step_local's clean workspace), and the
    unfused pair stays for the per-kernel timing path.
    mode "separable": the exact O(N*D) density, canonical scores for every
    row and a plain top-k, on the row-major pool.
    The Selection carries ``counts`` ([U, C] uint8); ``votes`` is None."""
    if mode not in ("gram", "separable"):
        raise ValueError(f"density mode must be 'gram' or 'separable', not {mode!r}")
    unl = _as_index(unlabeled_idx, state.device)
    if int(unl.shape[0]) == 0:
        raise ValueError("unlabeled set is empty (the reference loop breaks here)")
    if mode == "separable":
        flags, unl, n_cand = state.row_flags(unl)
        kk = min(int(k), n_cand)
        loc = state.local_positions(unl)
        counts, _, _, _, scores, keys, _ = forest_score_multiclass_dw(
            state, forest, flags, state.density_exact(), DAL_DENSITY_EXACT, beta=beta, want_hi=False)
        idx, _ = topk_keys(keys, kk, state.row_base)
        sel_scores = scores[idx - state.row_base]
        state.check_status()
        return Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, counts=(counts, loc))
    C = int(forest.n_classes)
    after_exclude, state._excluded_since_step = state._excluded_since_step, False
    if (state.use_graphs and not after_exclude and density_fixed is None and state._density is not None
            and state._colsum is not None
            and state.row_base == 0 and state.n == state.n_total and state.events_off()):
        return _density_step_graph(state, unl, forest, min(int(k), int(unl.shape[0])), beta, n_classes=C)
    # warm (density cached): the score kernel reads the pool's blocked copy
    # (built by the first warm step); the cold step keeps the row-major kernel
    xb = (state.blocked_pool(forest, multiclass=True)
          if state._density is not None or density_fixed is not None else None)
    # the density GEMM goes to the GPU first; the host prepares the rest while it runs
    dens, colsum_ready = _density_for_step(state, density_fixed)
    flags, unl, n_cand = state.row_flags(unl)
    kk = min(int(k), n_cand)
    loc = state.local_positions(unl)
    if state.forest_events is None and state.select_events is None:
        # one C call, fused launches, for a cold step, a handed-in density or a
        # shard (the per-kernel timing path below keeps K2 / K3 apart)
        counts, scores, idx, sel_scores = dw_step_local(
            state, forest, flags, dens, device_multiclass_lut("entropy", forest.n_trees, state.device), kk, beta,
            state.colsum(), colsum_ready, xb=xb, n_classes=C)
        state.check_status(state.last_status)
        return Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, counts=(counts, loc))
    counts, _, entropy, row_index, scores, keys_lo, keys_hi = forest_score_multiclass_dw(
        state, forest, flags, dens, DAL_DENSITY_FIXED, density_err=density_error(state), beta=beta, want_hi=True,
        xb=xb)
    # the main stream joins the column sum inside the call, just before the re-rank
    idx, sel_scores, _ = dw_select_local(state, flags, row_index, keys_lo, keys_hi, entropy, kk, beta,
                                         state.colsum(), colsum_ready=colsum_ready)
    state.check_status(state.last_status)  # the word dw_select_local read (no second sync)
    return Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, counts=(counts, loc))


def _density_for_step(state: PoolState, density_fixed=None):
    """The fixed-point Gram density a density-weighted step scores with:
    (density, colsum_ready).  On a cold pool the Gram is queued here, first,
    and the canonical column sum (only the exact re-rank needs it) runs on a
    side stream AFTER it, beside the vote / score chain (beside the Gram
    itself it would slow the persistent Gram blocks); colsum_ready is then
    the event recorded behind it, else None."""
    if density_fixed is None and state._density is None and state._colsum is None and state.n:
        torch = _torch()
        # the fused prep also writes the canonical column-sum partials (the side
        # stream below then only reduces them: 56 us less per config-2 step than
        # computing them after the Gram) and zeroes the density accumulator
        acc = torch.empty(state.n_pad, dtype=torch.int64, device=state.device)
        state.gram_operand(with_partials=True, acc_zero=acc)
        state._acc_pre = acc
        dens = state.density_fixed()
        main = torch.cuda.current_stream(state.device)
        side = _side_stream(state.device)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            cs = state.colsum()
            colsum_ready = torch.cuda.Event()
            colsum_ready.record(side)
        cs.record_stream(main)
        return dens, colsum_ready
    return (state.density_fixed() if density_fixed is None else density_fixed), None


def density_step(state: PoolState, unlabeled_idx, forest: Forest, k: int, beta: float = 1.0,
                 density_fixed=None, mode: str = "gram") -> Selection:
    """One iteration of density_weighting.py:133-176 on the GPU:
    score = ent[v] * d^beta, descending; exact canonical selection.

    mode "gram": density from the fused MFMA Gram row-sum (the reference's
    N^2 algorithm) with an exact fp64 re-rank of the boundary candidates;
    mode "separable": density from the exact O(N*D) identity (scores are then
    canonical fp64 for every row and the top-k needs no re-rank)."""
    if mode == "separable":
        return _density_step_separable(state, unlabeled_idx, forest, k, beta)
    if mode != "gram":
        raise ValueError(f"density mode must be 'gram' or 'separable', not {mode!r}")
    unl = _as_index(unlabeled_idx, state.device)
    if int(unl.shape[0]) == 0:
        raise ValueError("unlabeled set is empty (the reference loop breaks here)")
    after_exclude, state._excluded_since_step = state._excluded_since_step, False
    if (state.use_graphs and not after_exclude and density_fixed is None and state._density is not None
            and state._colsum is not None
            and state.row_base == 0 and state.n == state.n_total and state.events_off()):
        return _density_step_graph(state, unl, forest, min(int(k), int(unl.shape[0])), beta)
    # warm (density cached): the score kernel reads the pool's blocked copy
    # (built by the first warm step); the cold step keeps the row-major kernel
    xb = state.blocked_pool(forest) if state._density is not None or density_fixed is not None else None
    # the density GEMM goes to the GPU first; the host prepares the rest while it runs
    dens, colsum_ready = _density_for_step(state, density_fixed)
    flags, unl, n_cand = state.row_flags(unl)
    kk = min(int(k), n_cand)
    loc = state.local_positions(unl)
    lut_dev = device_lut("entropy", forest.n_trees, state.device)
    if (state.forest_events is None and state.select_events is None and state.row_base == 0
            and state.n == state.n_total):
        # one C call, fused launches (the per-kernel timing path below keeps K2 / K3 apart)
        votes, scores, idx, sel_scores = dw_step_local(state, forest, flags, dens, lut_dev, kk, beta,
                                                       state.colsum(), colsum_ready, xb=xb)
        state.check_status(state.last_status)
        return Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, votes=(votes, loc))
    votes, scores, keys_lo, keys_hi = forest_score(
        state, forest, lut_dev, flags, DAL_DESCENDING, density=dens,
        density_err=density_error(state), beta=beta, want_hi=True, xb=xb)
    # the main stream joins the column sum inside the call, just before the re-rank
    idx, sel_scores, _ = dw_select_local(state, flags, votes, keys_lo, keys_hi, lut_dev, kk, beta,
                                         state.colsum(), colsum_ready=colsum_ready)
    state.check_status(state.last_status)  # the word dw_select_local read (no second sync)
    if state.select_events is not None and state.step_select_probe is not None and state.level1_fast:
        state.step_select_probe(state, forest, flags, dens, lut_dev, kk, beta, xb)
    return Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, votes=(votes, loc))


class WarmStepGraph:
    """One warm density-weighted step (density cached -- the reference's
    per-iteration path, density_weighting.py:133-176) as a libdal plan
    (dal_dw_plan_create): dal_dw_step -- forest votes + score + interval
    keys, the candidate search, the exact fp64 re-rank and the final sort,
    fused into 5 launches -- captured once as a hipGraph over static device
    buffers.  Per step ONE C call (dal_dw_plan_run) rebuilds the row flags
    from the pool's base flags and the unlabeled list, replays the graph,
    copies the selection out and reads the status word.  A different forest
    is copied into the static heap arrays first.

    ``n_classes`` (None: the binary step) makes it the C-class plan
    (dal_dw_plan_create_multiclass: dal_dw_step_multiclass captured the same
    way): per-class ``counts`` [n, C] in the place of ``votes``, the per-row
    entropy and row index the re-rank reads, and the C-class blocked rule for
    the pool's blocked copy."""

    def __init__(self, state: PoolState, forest: Forest, k: int, beta: float, cap: int, passes: int,
                 colsum=None, packed=None, n_classes=None):
        """colsum: the canonical column sum to re-rank against (default the
        pool's own; a shard passes the global one).  packed: an int64 [3k+1]
        row receiving (selected keys | indices | score bits | status) -- the
        multi-GPU top-k all-gather row -- instead of the plan's own buffers."""
        import ctypes

        torch = _torch()
        dev = state.device
        n = state.n
        self.state, self.k, self.cap, self.passes = state, int(k), int(cap), int(passes)
        self.n_classes = None if n_classes is None else int(n_classes)
        multi = self.n_classes is not None
        forest.check_features(state.d)
        if multi:
            forest.check_classes()
            if forest.n_trees > DAL_MC_MAX_TREES:
                raise ValueError(
                    f"a multiclass forest may hold at most {DAL_MC_MAX_TREES} trees, not {forest.n_trees}")
        inner, leaf = forest.device(dev)
        self.inner, self.leaf = inner.clone(), leaf.clone()
        self.forest_ref = forest
        self.n_trees, self.depth = forest.n_trees, forest.depth
        self.flags = state.flags.clone()
        if multi:
            self.lut = device_multiclass_lut("entropy", forest.n_trees, dev)
            self.votes = None
            self.counts = torch.empty((n, self.n_classes), dtype=torch.uint8, device=dev)
            self.entropy = torch.empty(n, dtype=torch.float64, device=dev)
            self.row_index = torch.empty(n, dtype=torch.int32, device=dev)
        else:
            self.lut = device_lut("entropy", forest.n_trees, dev)
            self.votes = torch.empty(n, dtype=torch.int32, device=dev)
        self.scores = torch.empty(n, dtype=torch.float64, device=dev)
        self.keys_lo = torch.empty(n, dtype=torch.int64, device=dev)
        self.keys_hi = torch.empty(n, dtype=torch.int64, device=dev)
        self.packed = packed
        if packed is None:
            # selected indices and scores side by side: one copy hands them out
            self.out_pair = torch.empty(2 * k, dtype=torch.int64, device=dev)
            self.out_keys = torch.empty(k, dtype=torch.int64, device=dev)
            status = state.status
        else:
            if packed.dtype != torch.int64 or tuple(packed.shape) != (3 * k + 1,) or not packed.is_contiguous():
                raise ValueError("packed must be a contiguous int64 [3k+1] tensor")
            packed.zero_()  # the status slot's upper half stays zero
            self.out_keys, self.out_pair = packed[:k], packed[k:3 * k]
            status = packed[3 * k:].view(torch.int32)[:1]  # low half of the last word (little endian)
        self.status = status
        self._last = None  # weak reference to the Selection that still reads votes / scores
        lib = _lib.load()
        self.wsb = int(lib.dal_dw_step_workspace_bytes(n, k, cap))
        self.ws, self.wsp = workspace(self.wsb, dev)
        # the score kernel reads the pool's blocked copy when it applies
        xb = state.blocked_pool(forest, multiclass=True) if multi else state.blocked_pool(forest)
        # the forest prepared for the blocked kernel, in a static buffer the
        # plan reads at its captured address (re-prepared when the forest changes)
        self.fprep = None
        if xb is not None:
            nb = int(lib.dal_forest_prep_bytes(state.d, self.n_trees, self.depth))
            if nb:
                self.fprep = torch.empty(nb, dtype=torch.uint8, device=dev)
                self._prepare()
        self._keep = (state.density_fixed(), state.colsum() if colsum is None else colsum, state.norms(),
                      state.flags, state.x, xb)
        dens, colsum, norm64 = self._keep[:3]
        plan = ctypes.c_void_p()
        head = (_ptr(state.x), 0 if xb is None else _ptr(xb), 0 if self.fprep is None else _ptr(self.fprep), n,
                state.d, state.d, _ptr(self.inner), _ptr(self.leaf), self.n_trees, self.depth)
        step = (_ptr(self.lut), _ptr(dens), float(density_error(state)), _ptr(state.flags), _ptr(self.flags),
                float(beta), state.row_base, _ptr(norm64), _ptr(colsum), k, cap, passes, self.wsp, self.wsb)
        tail = (_ptr(self.scores), _ptr(self.keys_lo), _ptr(self.keys_hi), _ptr(self.out_pair), _ptr(self.out_keys),
                _ptr(status), _stream(dev), ctypes.byref(plan))
        if multi:  # (pred is not kept: a Selection carries the counts)
            call("dal_dw_plan_create_multiclass", *head, self.n_classes, *step, _ptr(self.counts), 0,
                 _ptr(self.entropy), _ptr(self.row_index), *tail)
        else:
            call("dal_dw_plan_create", *head, *step, _ptr(self.votes), *tail)
        self.plan = plan
        self._status = ctypes.c_int32()
        self._status_ref = ctypes.byref(self._status)
        self._run = lib.dal_dw_plan_run
        self._finalizer = weakref.finalize(self, lib.dal_dw_plan_destroy, plan)

    def _prepare(self):
        """dal_forest_prepare of the plan's static forest copy into its static
        prepared buffer (stream-ordered before the next replay)."""
        if self.fprep is not None:
            call("dal_forest_prepare", _ptr(self.inner), _ptr(self.leaf), self.n_trees, self.depth, self.state.d,
                 _ptr(self.fprep), int(self.fprep.shape[0]), _stream(self.state.device))

    def run(self, forest: Forest, unl):
        """Refresh the inputs, replay, read the status: returns (votes --
        the C-class plan: counts --, scores, selected indices, selected
        scores, status).  votes / scores are the plan's buffers, valid until
        the next replay (copy-on-write: the previous step's Selection is
        materialised before they are reused); the selection lands in fresh
        tensors."""
        torch = _torch()
        prev = self._last() if self._last is not None else None
        if prev is not None:
            prev._detach()
        dev = self.state.device
        if forest is not self.forest_ref:
            forest.check_features(self.state.d)
            if self.n_classes is not None:
                forest.check_classes()
            inner, leaf = forest.device(dev)
            self.inner.copy_(inner)
            self.leaf.copy_(leaf)
            self._prepare()
            self.forest_ref = forest
        idx = torch.empty(self.k, dtype=torch.int64, device=dev)
        sc = torch.empty(self.k, dtype=torch.float64, device=dev)
        rc = self._run(self.plan, unl.data_ptr(), unl.shape[0], idx.data_ptr(), sc.data_ptr(), self._status_ref,
                       _raw_stream(dev))
        if rc:
            _lib.check(rc, "dal_dw_plan_run")
        return (self.votes if self.n_classes is None else self.counts), self.scores, idx, sc, self._status.value

    def launch(self, forest: Forest, unl):
        """Refresh and replay on the current stream WITHOUT waiting (the
        outputs land in ``packed``); the caller reads the status later."""
        if forest is not self.forest_ref:
            forest.check_features(self.state.d)
            inner, leaf = forest.device(self.state.device)
            self.inner.copy_(inner)
            self.leaf.copy_(leaf)
            self._prepare()
            self.forest_ref = forest
        call("dal_dw_plan_launch", self.plan, unl.data_ptr(), int(unl.shape[0]), _raw_stream(self.state.device))


def _density_step_graph(state: PoolState, unl, forest: Forest, kk: int, beta: float, n_classes=None) -> Selection:
    """Warm density step through a cached WarmStepGraph (same selection as
    the eager path; a level-1 or re-rank capacity overflow rebuilds the plan
    with the exact level 1 / a larger capacity and replays).  ``n_classes``:
    the C-class step (its plans are cached beside the binary ones, by C)."""
    n = state.n
    loc = state.local_positions(unl)
    while True:
        base = candidate_cap(n, kk) if state.cap_base is None else max(int(kk), int(state.cap_base))
        cap = int(min(n, base * state.cap_scale))
        passes = level1_passes(state, n, kk, cap)
        key = (forest.n_trees, forest.depth, kk, float(beta), cap, passes)
        if n_classes is not None:
            key += (int(n_classes),)
        g = state._graphs.get(key)
        if g is None:
            g = state._graphs[key] = WarmStepGraph(state, forest, kk, beta, cap, passes, n_classes=n_classes)
        try:
            votes, scores, idx, sel_scores, st = g.run(forest, unl)
        except _lib.DalError:
            # a failed replay may leave the plan's workspace header dirty: rebuild next time
            state._graphs.pop(key, None)
            raise
        state.last_status = st
        if st & DAL_FLAG_SAMPLE_MISS:
            state.status.bitwise_and_(~(DAL_FLAG_SAMPLE_MISS | DAL_FLAG_CAND_OVERFLOW))
            state.level1_fast = False
            continue
        if (st & DAL_FLAG_CAND_OVERFLOW) and cap < n:
            state.status.bitwise_and_(~DAL_FLAG_CAND_OVERFLOW)
            state.cap_scale *= 4
            continue
        state.check_status(st)
        if n_classes is None:
            sel = Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, votes=(votes, loc))
        else:
            sel = Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, counts=(votes, loc))
        g._last = weakref.ref(sel)
        return sel


def torch_float64():
    return _torch().float64


def _density_step_separable(state: PoolState, unlabeled_idx, forest: Forest, k: int,
                            beta: float) -> Selection:
    flags, unl, n_cand = state.row_flags(unlabeled_idx)
    if n_cand == 0:
        raise ValueError("unlabeled set is empty (the reference loop breaks here)")
    kk = min(int(k), n_cand)
    loc = state.local_positions(unl)
    lut_dev = device_lut("entropy", forest.n_trees, state.device)
    votes, scores, keys, _ = forest_score(state, forest, lut_dev, flags, DAL_DESCENDING,
                                          density=state.density_exact(), beta=beta)
    idx, _ = topk_keys(keys, kk, state.row_base)
    sel_scores = scores[idx - state.row_base]
    state.check_status()
    return Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, votes=(votes, loc))


# ------------------------------------------------------------------ LAL --
def forest_regress(model, x, n: int, d: int, ldx: int, device, f64: bool):
    """Launch dal_forest_regress over n rows of ``x`` (a device tensor, fp32
    or fp64 by ``f64``): the regression forest's prediction, fp64 [n]."""
    torch = _torch()
    model.check_features(d)
    feat, thr, leaf = model.device(device)
    out = torch.empty(n, dtype=torch.float64, device=device)
    call("dal_forest_regress", _ptr(x), _lib.DAL_X_F64 if f64 else _lib.DAL_X_F32, n, d, ldx, _ptr(feat), _ptr(thr),
         _ptr(leaf), model.n_trees, model.depth, _ptr(out), _stream(device))
    return out


def device_lal_tables(n_trees: int, device):
    """(f1, f2) of dal.active_learner.lal_tables on the device, uploaded once
    per (T, device)."""
    torch = _torch()
    key = ("lal", int(n_trees), str(device))
    if key not in _LUT_CACHE:
        from .active_learner import lal_tables

        _LUT_CACHE[key] = tuple(torch.from_numpy(t).to(device) for t in lal_tables(n_trees))
    return _LUT_CACHE[key]


def lal_votes(state: PoolState, forest: Forest, flags):
    """The LAL step's first half on one shard: the forest votes of every row
    (dal_forest_score; its scores and keys, written for a stand-in LUT, are
    dropped) and the vote histogram of the candidates, int64 [T + 1]."""
    torch = _torch()
    T = forest.n_trees
    lut0 = device_lut("least_confidence", T, state.device)  # any LUT: only the votes are kept
    votes, _, _, _ = forest_score(state, forest, lut0, flags, DAL_ASCENDING, xb=uncertainty_blocked(state, forest))
    hist = torch.zeros(T + 1, dtype=torch.int64, device=state.device)
    call("dal_vote_histogram", _ptr(votes), _ptr(flags), state.n, T, _ptr(hist), _stream(state.device))
    return votes, hist


def lal_scores(state: PoolState, forest: Forest, lal_model, flags, votes, hist, n_labeled: int, n_positive: int):
    """The LAL step's second half, from the (all-reduced) histogram: the T + 1
    feature rows, the regressor over them (the LUT), and every row's score and
    descending key.  Returns (lut [T + 1], scores [n], keys [n])."""
    torch = _torch()
    dev = state.device
    T = forest.n_trees
    f1, f2 = device_lal_tables(T, dev)
    rows = torch.empty((T + 1, 5), dtype=torch.float64, device=dev)
    call("dal_lal_rows", _ptr(hist), _ptr(f1), _ptr(f2), T, float(n_positive) / n_labeled, float(n_labeled),
         _ptr(rows), _stream(dev))
    lut = forest_regress(lal_model, rows, T + 1, 5, 5, dev, f64=True)
    scores = torch.empty(state.n, dtype=torch.float64, device=dev)
    keys = torch.empty(state.n, dtype=torch.int64, device=dev)
    call("dal_votes_rescore", _ptr(votes), _ptr(flags), state.n, _ptr(lut), T, DAL_DESCENDING, _ptr(scores),
         _ptr(keys), _stream(dev))
    return lut, scores, keys


def check_lal_inputs(forest: Forest, lal_model, n_labeled, n_positive):
    """The LAL step's argument rules (pure host code)."""
    if forest.n_classes > 2:
        raise ValueError(f"LAL is binary only: the forest has {forest.n_classes} classes")
    if not 2 <= forest.n_trees <= _lib.DAL_LAL_MAX_TREES:
        raise ValueError(f"LAL needs a forest of 2..{_lib.DAL_LAL_MAX_TREES} trees (getSD divides by T - 1), "
                         f"not {forest.n_trees}")
    if int(n_labeled) < 1:
        raise ValueError("n_labeled must be at least 1")
    if not 0 <= int(n_positive) <= int(n_labeled):
        raise ValueError("n_positive must lie in [0, n_labeled]")
    lal_model.check_features(5)


def lal_step(state: PoolState, unlabeled_idx, forest: Forest, lal_model, k: int, n_labeled: int,
             n_positive: int) -> Selection:
    """One iteration of ActiveLearnerLAL.selectNext (active_learner.py:247-334)
    on the GPU: votes -> histogram -> feature rows -> regressor -> rescore ->
    top-k (descending, the largest predicted error reduction), every launch
    stream-ordered.  The Selection also carries ``lut`` (fp64 [T + 1])."""
    check_lal_inputs(forest, lal_model, n_labeled, n_positive)
    flags, unl, n_cand = state.row_flags(unlabeled_idx)
    if n_cand == 0:
        raise ValueError("unlabeled set is empty (the reference loop breaks here)")
    kk = min(int(k), n_cand)
    loc = state.local_positions(unl)
    votes, hist = lal_votes(state, forest, flags)
    lut, scores, keys = lal_scores(state, forest, lal_model, flags, votes, hist, n_labeled, n_positive)
    idx, _ = topk_keys(keys, kk, state.row_base)
    sel_scores = scores[idx - state.row_base]
    state.check_status()
    sel = Selection(scores=(scores, loc), indices=idx, selected_scores=sel_scores, votes=(votes, loc))
    sel.lut = lut
    return sel
