"""Row-sharded multi-GPU query selection (one process per GPU, RCCL over xGMI).

Reference parallelism: Spark data parallelism over RDD row partitions, with
the cross-partition steps done as shuffles:
BlockMatrix.multiply's block cogroup (density_weighting.py:73), groupByKey
(:144, :159) and sortBy + take to the driver (:168, :172).

Here the pool is row-sharded in contiguous shards of ``shard`` rows (a
multiple of DAL_ROW_GRANULE, identical on every rank; the last rank holds the
remainder).  Two exchanges, both all-gathers over ``torch.distributed``
(backend "nccl" = RCCL on ROCm):

  1. the shards' Gram operands (fp16 split [shard, 2*d_pad] by default, or
     fp32 unit rows) and the canonical fp64 column-sum partials -> every rank
     holds U (the density needs every column; the symmetric kernel's
     closed-form remainder needs every super block's row sums) -- replaces
     the BlockMatrix shuffle.  The operand all-gather runs asynchronously on RCCL's stream
     while each rank multiplies its rows by its OWN shard's columns (CUs
     reserved for RCCL), then by the rest (ShardedSelector.exchange_density);
  2. each rank's exact local top-k (key, index, score) -> an identical
     deterministic merge on every rank -- replaces sortBy + take.

Determinism: global row r sits at column r of the gathered U on every P, the
density is accumulated in exact int64 fixed point, and the canonical column
sum is reduced over the same 256-row chunks in the same order, so every
density bit, every score and the selected set are identical for P = 1..8.

Every sharded operation has ONE body, over a list of jobs and an ``ops``
object that supplies the collectives: a rank calls it with its one job and
_GroupOps (the real group), the ``emulate_*`` functions with P jobs in one
process and _LocalOps (sums, stacks, concatenations), so a test that drives P
emulated shards on the GPU runs the code the ranks run.  The local phases are
selector methods, which the CPU tests replace with the oracle.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import DAL_ASCENDING, DAL_CANON_CHUNK, DAL_DESCENDING, DAL_KEY_NONE, DAL_ROW_GRANULE

# CUs left to RCCL while the own-shard Gram launch runs beside the all-gather
# (a persistent Gram grid would otherwise hold every CU's registers and LDS).
RCCL_RESERVED_CUS = 8

# selection modes that score with the density: "dw" (binary, the reference's
# one-sided entropy) and "dw_multiclass" (class entropy, any C >= 2) over hard
# votes, and "dw_soft" (the entropy of a ProbabilityForest's averaged leaf
# distributions) over soft votes
DENSITY_MODES = ("dw", "dw_multiclass")
SOFT_DENSITY_MODES = ("dw_soft",)
ALL_DENSITY_MODES = DENSITY_MODES + SOFT_DENSITY_MODES


def _soft_forest(forest, mode: str, strategy: str = None) -> bool:
    """True for a dal.forest.ProbabilityForest (soft votes), which modes "us"
    and "dw_soft" alone score; any other mode raises ValueError, before any
    work -- as does mode "dw_soft" for a hard-voting Forest."""
    from .forest import ProbabilityForest

    soft = isinstance(forest, ProbabilityForest)
    if strategy == "bald" and mode == "us" and not soft:
        raise ValueError("strategy='bald' (the trees' disagreement) needs a ProbabilityForest (soft votes): a "
                         "hard-voting Forest keeps no leaf distributions")
    if soft and mode != "us" and mode not in SOFT_DENSITY_MODES:
        raise ValueError(f"a ProbabilityForest (soft votes) is scored by mode='us' or mode='dw_soft' only: "
                         f"mode={mode!r} has no soft-vote form (the hard-vote density-weighted and LAL scores take "
                         "hard votes; forest.hard() gives the hard-voting Forest)")
    if mode in SOFT_DENSITY_MODES and not soft:
        raise ValueError("mode='dw_soft' scores a ProbabilityForest (soft votes): a hard-voting Forest belongs to "
                         "mode='dw' (binary) or mode='dw_multiclass'")
    return soft


def shard_rows(n_total: int, world: int) -> int:
    """Rows per shard: ceil(N / P) rounded up to the row granule (512)."""
    per = -(-n_total // world)
    return -(-per // DAL_ROW_GRANULE) * DAL_ROW_GRANULE


def shard_range(n_total: int, world: int, rank: int):
    s = shard_rows(n_total, world)
    lo = min(rank * s, n_total)
    hi = min(lo + s, n_total)
    return lo, hi, s


@dataclass
class LocalTopk:
    """A rank's exact local top-k, padded to k with DAL_KEY_NONE."""

    keys: object  # int64 [k] (uint64 bit patterns)
    idx: object  # int64 [k] global row indices
    scores: object  # fp64 [k]

    @classmethod
    def empty(cls, k: int, device):
        """k padding slots: DAL_KEY_NONE, index -1, score NaN."""
        torch = __import__("torch")
        return cls(torch.full((k,), _as_i64(DAL_KEY_NONE), dtype=torch.int64, device=device),
                   torch.full((k,), -1, dtype=torch.int64, device=device),
                   torch.full((k,), float("nan"), dtype=torch.float64, device=device))


def merge_topk(keys_all, idx_all, scores_all, k: int, sort_fn, all_valid: bool = False):
    """Deterministic merge of P gathered local top-k lists (rank-major).

    Each list is sorted by (key, index) and shards are in global index order,
    so sorting by (key, position) orders ties by global index; ``sort_fn``
    returns the positions of the k best.  ``all_valid``: at least k candidates
    exist globally, so no padding key can reach the k best and the filter
    (a host sync) is skipped."""
    torch = __import__("torch")
    n = int(keys_all.shape[0])
    pos = torch.arange(n, dtype=torch.int64, device=keys_all.device)
    best = sort_fn(keys_all, pos, k)
    if not all_valid:
        valid = keys_all[best] != _as_i64(DAL_KEY_NONE)
        best = best[valid]
    return idx_all[best], scores_all[best]


def _as_i64(u: int) -> int:
    return u - (1 << 64) if u >= (1 << 63) else u


class ShardedSelector:
    """One rank's shard of the pool and its share of a selection step."""

    def __init__(self, x_local, n_total: int, rank: int, world: int, excluded=None, device=None,
                 gram: str = None, gram_i8=None, gram_fp4=None):
        from .engine import PoolState

        self.n_total, self.rank, self.world = int(n_total), int(rank), int(world)
        self.lo, self.hi, self.shard = shard_range(self.n_total, self.world, self.rank)
        if int(x_local.shape[0]) != self.hi - self.lo:
            raise ValueError(f"rank {rank}: expected {self.hi - self.lo} rows, got {x_local.shape[0]}")
        self.state = PoolState(x_local, excluded=excluded, device=device, row_base=self.lo,
                               n_total=self.n_total, n_pad=self.shard, gram=gram, gram_i8=gram_i8, gram_fp4=gram_fp4)
        self._density = None
        self._parts_full = None  # all ranks' canonical column-sum partials (cached with the density)
        self._colsum = None      # the global canonical column sum reduced from them (cached)
        self._plans = {}         # warm-step plans by (T, depth, k, beta, cap, level-1 passes)
        self.cap_scale = 1      # re-rank candidate capacity multiplier (grown on overflow)
        # bench: list -> (name, start, end) HIP events around the density
        # exchange's collective ("all_gather": operand + partials, recorded on
        # the stream that waits for them)
        self.exchange_events = None

    def index_tensor(self, unlabeled_idx):
        from .engine import _as_index

        return _as_index(unlabeled_idx, self.state.device)

    def status_word(self):
        """This rank's device status word (DAL_FLAG_* bits), int32 [1]."""
        return self.state.status

    def prepare_retry(self, sample_miss: bool = False):
        """After a re-rank capacity overflow (or a fast level-1
        overflow) anywhere: grow the capacity (or fall back to the exact radix
        level 1) and go again.  The density, operand and column-sum caches stay valid,
        so the retry does not redo the Gram."""
        self.state.status.zero_()
        if sample_miss:
            self.state.level1_fast = False
        else:
            self.cap_scale *= 4

    def clear_caches(self):
        """Drop the shard's normalised rows, density and column sums (cold step)."""
        self.state.clear_caches()
        self._density = None
        self._parts_full = None
        self._colsum = None
        self._plans = {}

    def global_colsum(self, partials_full):
        """The canonical column sum s = sum_{j not in E} u_j over EVERY rank's
        rows, reduced once from the gathered partials and cached (a warm-step
        plan captures its address)."""
        if self._colsum is None or partials_full is not self._parts_full:
            cs = self.state.colsum(partials_full)
            if partials_full is not self._parts_full:
                return cs
            self._colsum = cs
        return self._colsum

    def warm_plan(self, forest, k: int, beta: float):
        """This rank's warm local step (density cached) as a dal_dw_plan whose
        outputs land in one packed row [keys k | indices k | score bits k |
        status]: launched without a host wait, all-gathered and merged
        stream-ordered (engine.WarmStepGraph with ``packed``)."""
        from .engine import WarmStepGraph, candidate_cap, level1_passes

        torch = __import__("torch")
        st = self.state
        base = candidate_cap(st.n, k) if st.cap_base is None else max(int(k), int(st.cap_base))
        cap = int(min(st.n, base * self.cap_scale))
        passes = level1_passes(st, st.n, k, cap)
        key = (forest.n_trees, forest.depth, int(k), float(beta), cap, passes)
        g = self._plans.get(key)
        if g is None:
            packed = torch.empty(3 * int(k) + 1, dtype=torch.int64, device=st.device)
            g = self._plans[key] = WarmStepGraph(st, forest, int(k), beta, cap, passes,
                                                 colsum=self.global_colsum(self._parts_full), packed=packed)
        return g

    # ---- phase A: local normalisation + canonical partials ------------
    def prep(self):
        """(Gram operand of the shard -- fp32 unit rows [shard, d_pad] or their
        fp16 split [shard, 2*d_pad] --, partials [shard/256, d] fp64)."""
        torch = __import__("torch")
        st = self.state
        u = st.gram_operand()
        parts = torch.zeros((self.shard // DAL_CANON_CHUNK, st.d), dtype=torch.float64,
                            device=st.device)
        if st.n:
            p = st.colsum_partials()
            parts[: p.shape[0]] = p
        return u, parts

    # ---- exchange 1 overlapped with the own-shard columns ---------------
    def exchange_density(self, comm, u_local, parts=None, reserve_cus: int = RCCL_RESERVED_CUS):
        """All-gather the shards' Gram operands (and the canonical partials)
        while this rank's rows run against its OWN columns (the operand it
        already holds), then against the other shards' columns; returns
        (gathered operand, gathered partials).  Every column range is a whole
        number of shards (multiples of 512), so the exact fixed-point sum is the
        same bits as one call over all columns.

        With RCCL (``comm.overlaps``) the own-shard Gram is queued FIRST, on
        all but ``reserve_cus`` CUs, and the collectives are enqueued behind it
        from a side stream that only waits for the operand -- the host's
        collective-issue time runs under the Gram instead of in front of it.
        gram "sym": the accumulator is indexed by global row; this rank's
        pairs yield row sums of its own rows only (the column sums of the pairs
        that take its rows come from the closed-form residual), so no density
        collective follows the all-gather."""
        torch = __import__("torch")
        st = self.state
        acc = self._new_acc()
        if getattr(comm, "overlaps", False) and st.n:
            main = torch.cuda.current_stream(st.device)
            ready = main.record_event()
            grid = max(1, 2 * (_device_cus(st.device) - reserve_cus))
            st.gram_accumulate(acc, u_local, self.shard, grid_blocks=grid, col_row0=self.lo)
            side = _side_stream(st.device)
            side.wait_event(ready)
            with torch.cuda.stream(side):
                ev = self._event_start("all_gather")
                parts_full, pwork = comm.all_gather_start(parts) if parts is not None else (None, None)
                u_full, work = comm.all_gather_start(u_local)
                if ev is not None:  # the side stream waits for the collectives, then records
                    comm.wait(work)
                    comm.wait(pwork)
                    self._event_end(ev)
            for t in (u_full, parts_full):
                if t is not None:
                    t.record_stream(main)
            main.wait_stream(side)
            comm.wait(work)   # the current (main) stream waits for the collectives
            comm.wait(pwork)
        else:
            ev = self._event_start("all_gather")
            parts_full, pwork = comm.all_gather_start(parts) if parts is not None else (None, None)
            u_full, work = comm.all_gather_start(u_local)
            if ev is not None:
                if work is None and pwork is None:  # staged (gloo): already complete
                    self._event_end(ev)
                else:  # the end on a side stream that waits for the collectives only (not the Gram below)
                    side = _side_stream(st.device)
                    side.wait_stream(torch.cuda.current_stream(st.device))
                    with torch.cuda.stream(side):
                        comm.wait(work)
                        comm.wait(pwork)
                        self._event_end(ev)
                ev = None
            if st.n:
                st.gram_accumulate(acc, u_local, self.shard, col_row0=self.lo)
            comm.wait(work)
            comm.wait(pwork)
        if st.n and self.world > 1:
            if st.gram == "sym":  # one launch over every other column
                st.gram_accumulate(acc, u_full, self.world * self.shard, col_row0=0,
                                   skip=(self.lo, self.lo + self.shard))
            else:
                for c0, c1 in other_column_ranges(self.rank, self.world, self.shard):
                    st.gram_accumulate(acc, u_full[c0:c1], c1 - c0, col_row0=c0)
        if st.gram == "sym":
            if st.n:  # the closed-form remainder and column sums of this rank's rows
                st.gram_residual(acc, u_full)
            acc = self._own_rows(acc)
        self.set_density(acc)
        return u_full, parts_full

    def _own_rows(self, acc):
        """gram "sym": the kernel adds the row sums of the pairs this rank's
        super blocks take and the residual adds every other part of its rows
        (the column sums of the pairs that take them, in closed form), all at
        GLOBAL row indices of a [world * shard] accumulator -- nothing lands on
        another rank's rows, so the density is this rank's slice (no
        collective)."""
        return acc[self.rank * self.shard:(self.rank + 1) * self.shard]

    def _event_start(self, name):
        if self.exchange_events is None:
            return None
        torch = __import__("torch")
        ev = (name, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[1].record()
        return ev

    def _event_end(self, ev):
        if ev is not None:
            ev[2].record()
            self.exchange_events.append(ev)

    def _new_acc(self):
        torch = __import__("torch")
        n = self.world * self.shard if self.state.gram == "sym" else self.state.n_pad
        return torch.zeros(n, dtype=torch.int64, device=self.state.device)

    def density_contribution(self, u_full):
        """This rank's fixed-point density against every column of the
        gathered operand: its own rows' sums ([shard])."""
        acc = self._new_acc()
        if self.state.n:
            self.state.gram_accumulate(acc, u_full, int(u_full.shape[0]), col_row0=0)
            if self.state.gram == "sym":
                self.state.gram_residual(acc, u_full)
        return self._own_rows(acc) if self.state.gram == "sym" else acc

    def set_density(self, acc_local):
        self._density = acc_local
        self.state.set_density_fixed(acc_local)

    # ---- phase B: density against all columns + local exact top-k ------
    def local_density(self, u_full):
        if self._density is None:
            self.set_density(self.density_contribution(u_full))
        return self._density

    def local_select(self, u_full, partials_full, unlabeled_idx, forest, k: int, mode: str = "dw",
                     strategy: str = "least_confidence", beta: float = 1.0,
                     density_mode: str = "gram", warm: bool = None) -> LocalTopk:
        """This rank's exact local top-k.  mode: "us" (uncertainty), "dw"
        (binary density weighting), "dw_multiclass" (class entropy x
        density, any forest of two or more classes; the C-class score kernel
        and dal_dw_select) or "dw_soft" (entropy of the averaged leaf
        distributions x density: a dal.forest.ProbabilityForest alone, through
        dal_dw_step_soft).  A ProbabilityForest (soft votes) is scored by
        modes "us" and "dw_soft" alone; every other mode raises ValueError.
        Mode "us" over such a forest also takes strategy="bald" (the trees'
        disagreement, dal_forest_score_soft_bald; a row's score does not
        depend on the shard, so the merge is the same).
        ``warm``: the density was cached
        before this step (the score kernel then reads the shard's blocked
        copy, as the single-GPU warm step does; a cold step keeps the
        row-major kernel and builds no copy).  None: cached now."""
        from .engine import (density_error, device_lut, dw_select_local, dw_step_local, forest_score,
                             topk_keys, uncertainty_blocked)
        from .luts import ASCENDING

        st = self.state
        soft = _soft_forest(forest, mode, strategy)
        if mode == "dw" and forest.n_classes > 2:
            raise ValueError(f"density weighting is binary only: the forest has {forest.n_classes} classes")
        if st.n == 0:
            return LocalTopk.empty(k, st.device)
        flags, unl, _ = st.row_flags(unlabeled_idx)
        # no host count of this shard's candidates (a sync): rows that are not
        # candidates carry the padding key, so with fewer than k candidates
        # they fill the local list last and never survive a merge that has k
        kk = min(k, st.n)
        if mode == "dw" and density_mode == "separable":
            colsum = self.global_colsum(partials_full)
            lut_dev = device_lut("entropy", forest.n_trees, st.device)
            votes, sc, kys, _ = forest_score(st, forest, lut_dev, flags, DAL_DESCENDING,
                                             density=st.density_exact(colsum), beta=beta)
            i, kk_keys = topk_keys(kys, kk, st.row_base)
            s = sc[i - st.row_base]
        elif mode == "dw":
            # warm (density cached): the score kernel reads the shard's blocked copy, as on one GPU
            warm_now = self._density is not None if warm is None else warm
            xb = st.blocked_pool(forest) if warm_now else None
            dens = self.local_density(u_full)
            colsum = self.global_colsum(partials_full)
            lut_dev = device_lut("entropy", forest.n_trees, st.device)
            if st.events_off():  # one fused call (dal_dw_step), as the single-GPU step
                _, _, i, s, kk_keys = dw_step_local(st, forest, flags, dens, lut_dev, kk, beta, colsum,
                                                    cap_scale=self.cap_scale, sync=False, xb=xb)
            else:  # bench per-kernel timing: K2 and K3 as separate calls
                votes, sc, klo, khi = forest_score(st, forest, lut_dev, flags, DAL_DESCENDING, density=dens,
                                                   density_err=density_error(st), beta=beta, want_hi=True,
                                                   xb=xb)
                i, s, kk_keys = dw_select_local(st, flags, votes, klo, khi, lut_dev, kk, beta, colsum,
                                                cap_scale=self.cap_scale, sync=False)
        elif mode == "dw_multiclass":
            # class entropy x density (any C >= 2): the C-class score kernel's
            # density-weighted form (warm: over the shard's blocked copy, as
            # the binary branch), then the same exact selection with lut =
            # entropy, votes = the identity index
            from ._lib import DAL_DENSITY_EXACT, DAL_DENSITY_FIXED
            from .engine import forest_score_multiclass_dw

            colsum = self.global_colsum(partials_full)
            if density_mode == "separable":
                _, _, _, _, sc, kys, _ = forest_score_multiclass_dw(
                    st, forest, flags, st.density_exact(colsum), DAL_DENSITY_EXACT, beta=beta, want_hi=False)
                i, kk_keys = topk_keys(kys, kk, st.row_base)
                s = sc[i - st.row_base]
            else:
                warm_now = self._density is not None if warm is None else warm
                xb = st.blocked_pool(forest, multiclass=True) if warm_now else None
                dens = self.local_density(u_full)
                _, _, ent, rix, _, klo, khi = forest_score_multiclass_dw(
                    st, forest, flags, dens, DAL_DENSITY_FIXED, density_err=density_error(st), beta=beta,
                    want_hi=True, xb=xb)
                i, s, kk_keys = dw_select_local(st, flags, rix, klo, khi, ent, kk, beta, colsum,
                                                cap_scale=self.cap_scale, sync=False)
        elif mode == "dw_soft":
            # entropy(predict_proba) x density: the soft kernel's density-weighted
            # form on the row-major shard (it has no blocked form), then the same
            # exact selection with lut = entropy, votes = the identity index
            from ._lib import DAL_DENSITY_EXACT, DAL_DENSITY_FIXED
            from .engine import forest_score_soft_dw

            colsum = self.global_colsum(partials_full)
            if density_mode == "separable":
                _, _, _, _, sc, kys, _ = forest_score_soft_dw(
                    st, forest, flags, st.density_exact(colsum), DAL_DENSITY_EXACT, beta=beta, want_hi=False)
                i, kk_keys = topk_keys(kys, kk, st.row_base)
                s = sc[i - st.row_base]
            else:
                dens = self.local_density(u_full)
                if st.events_off():  # one fused call (dal_dw_step_soft), as the single-GPU step
                    _, _, i, s, kk_keys = dw_step_local(st, forest, flags, dens, None, kk, beta, colsum,
                                                        cap_scale=self.cap_scale, sync=False, soft=True)
                else:  # bench per-kernel timing: K2 and K3 as separate calls
                    _, _, ent, rix, _, klo, khi = forest_score_soft_dw(
                        st, forest, flags, dens, DAL_DENSITY_FIXED, density_err=density_error(st), beta=beta,
                        want_hi=True)
                    i, s, kk_keys = dw_select_local(st, flags, rix, klo, khi, ent, kk, beta, colsum,
                                                    cap_scale=self.cap_scale, sync=False)
        elif soft:  # soft votes: the averaged leaf distributions, the same merge
            from .engine import SOFT_KINDS, forest_score_soft, forest_score_soft_bald
            from .luts import MULTICLASS_ASCENDING

            if strategy == "bald":  # the trees' disagreement: a row's score does not depend on the shard
                _, _, _, _, sc, kys = forest_score_soft_bald(st, forest, flags, DAL_DESCENDING)
            else:
                order = DAL_ASCENDING if MULTICLASS_ASCENDING[strategy] else DAL_DESCENDING
                _, _, sc, kys = forest_score_soft(st, forest, flags, order, SOFT_KINDS[strategy])
            i, kk_keys = topk_keys(kys, kk, st.row_base)
            s = sc[i - st.row_base]
        elif forest.n_classes > 2:  # multiclass uncertainty: the C-class kernel, the same merge
            from .engine import MULTICLASS_KINDS, device_multiclass_lut, forest_score_multiclass
            from .luts import MULTICLASS_ASCENDING

            order = DAL_ASCENDING if MULTICLASS_ASCENDING[strategy] else DAL_DESCENDING
            lut_dev = device_multiclass_lut(strategy, forest.n_trees, st.device)
            _, _, sc, kys = forest_score_multiclass(st, forest, lut_dev, flags, order, MULTICLASS_KINDS[strategy],
                                                    xb=uncertainty_blocked(st, forest, multiclass=True))
            i, kk_keys = topk_keys(kys, kk, st.row_base)
            s = sc[i - st.row_base]
        else:
            order = DAL_ASCENDING if ASCENDING[strategy] else DAL_DESCENDING
            lut_dev = device_lut(strategy, forest.n_trees, st.device)
            votes, sc, kys, _ = forest_score(st, forest, lut_dev, flags, order, xb=uncertainty_blocked(st, forest))
            i, kk_keys = topk_keys(kys, kk, st.row_base)
            s = sc[i - st.row_base]
        if kk == k:  # every slot written by the selection
            return LocalTopk(kk_keys, i, s)
        out = LocalTopk.empty(k, st.device)
        out.keys[:kk], out.idx[:kk], out.scores[:kk] = kk_keys, i, s
        return out


def other_column_ranges(rank: int, world: int, shard: int):
    """Column ranges [c0, c1) of the gathered operand outside this rank's own
    shard (at most two contiguous ranges: before and after it)."""
    out = []
    if rank > 0:
        out.append((0, rank * shard))
    if rank < world - 1:
        out.append(((rank + 1) * shard, world * shard))
    return out


def _device_cus(device) -> int:
    torch = __import__("torch")
    return int(torch.cuda.get_device_properties(device).multi_processor_count)


def hip_sort_positions(keys, pos, k):
    from .engine import sort_pairs

    _, out_pos, _ = sort_pairs(keys, pos, k)
    return out_pos


def _needs_bytes(dtype) -> bool:
    """Neither RCCL/NCCL nor gloo has torch's 16-bit integer or unsigned
    16/32/64-bit types (the split Gram operand is int16 bit patterns): such
    tensors are gathered as their bytes (a gather only moves bits)."""
    torch = __import__("torch")
    names = ("int16", "uint16", "uint32", "uint64")
    return any(getattr(torch, n, None) == dtype for n in names)


_SIDE_STREAMS = {}


def _side_stream(device):
    """A second stream per device from which collectives are enqueued behind
    an already queued Gram launch."""
    torch = __import__("torch")
    key = str(device)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


class TorchComm:
    """all-gather over torch.distributed (RCCL on ROCm GPUs, gloo on CPU)."""

    def __init__(self, group=None):
        import torch.distributed as dist

        self.dist = dist
        self.group = group
        self.world = dist.get_world_size(group)
        self.backend = dist.get_backend(group)
        # RCCL collectives are asynchronous on their own stream: they can run
        # beside a Gram launch (gloo stages through the host synchronously)
        self.overlaps = self.backend == "nccl"
        self._rows = {}  # (width, device) -> the merge's gathered-rows buffer

    def all_gather_rows(self, row):
        """All-gather one int64 row per rank into a buffer kept for the next
        step ([P, w]; its previous contents were consumed by the previous
        merge, which the step's status read waited for).  The warm multi-GPU
        step's collective, with the fewest host calls (RCCL: enqueued on the
        communicator's stream, ordered before the current stream's next work)."""
        torch = __import__("torch")
        if not row.is_cuda or self.backend == "gloo":
            return self.all_gather(row.reshape(1, -1))
        w = int(row.shape[0])
        key = (w, row.device)
        out = self._rows.get(key)
        if out is None:
            out = self._rows[key] = torch.empty((self.world, w), dtype=row.dtype, device=row.device)
        self.dist.all_gather_into_tensor(out, row, group=self.group)
        return out

    def all_gather(self, t):
        out, work = self.all_gather_start(t)
        self.wait(work)
        return out

    def all_gather_start(self, t):
        """Start an all-gather; returns (output, work handle or None).  With
        RCCL it runs asynchronously on the communicator's stream."""
        torch = __import__("torch")
        if t.dim() and _needs_bytes(t.dtype):
            out, work = self.all_gather_start(t.contiguous().view(torch.uint8))
            return out.view(t.dtype), work
        if t.is_cuda and self.backend == "gloo":
            # rehearsal path (several ranks sharing one GPU): stage through the host
            return self.all_gather(t.cpu()).to(t.device), None
        out = torch.empty((self.world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        if t.is_cuda:
            work = self.dist.all_gather_into_tensor(out, t.contiguous(), group=self.group, async_op=True)
            return out, work
        self.dist.all_gather_into_tensor(out, t.contiguous(), group=self.group)
        return out, None

    def wait(self, work):
        """Order the current stream after the collective (no host block)."""
        if work is not None:
            work.wait()


class _GroupOps:
    """The collectives of a sharded operation over a real group (one local job)."""

    def __init__(self, comm):
        self.comm = comm

    def reduce(self, tensors, op: str):
        dist = self.comm.dist
        ops = {"sum": dist.ReduceOp.SUM, "min": dist.ReduceOp.MIN, "max": dist.ReduceOp.MAX}
        dist.all_reduce(tensors[0], op=ops[op], group=self.comm.group)  # in place, stream-ordered
        return tensors

    def gather_rows(self, tensors):
        """Every rank's rows [c_r, w] as one [sum c_r, w]: the counts first,
        then the rows padded to the largest count."""
        torch = __import__("torch")
        t = tensors[0]
        counts = self.comm.all_gather(torch.tensor([t.shape[0]], dtype=torch.int64, device=t.device)).cpu().tolist()
        top = max(counts)
        pad = torch.zeros((top,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        pad[:t.shape[0]] = t
        got = self.comm.all_gather(pad).reshape((len(counts), top) + tuple(t.shape[1:]))
        return [torch.cat([got[r, :c] for r, c in enumerate(counts)])]

    def all_gather(self, tensors):
        """Every rank's block [m, ...] of ONE shape as [P * m, ...]: no counts, no host read."""
        return [self.comm.all_gather(tensors[0])]

    def gather_row(self, rows):
        """One int64 row per rank as [P, w] (TorchComm.all_gather_rows: stream-ordered, no host
        read; a comm without that method gathers the row as a [1, w] block)."""
        comm = self.comm
        if hasattr(comm, "all_gather_rows"):
            return [comm.all_gather_rows(rows[0])]
        return [comm.all_gather(rows[0].reshape(1, -1))]

    def exchange_density(self, sels, preps):
        """The operand / partials exchange beside the own-shard Gram
        (ShardedSelector.exchange_density); [(gathered operand, gathered partials)]."""
        return [sels[0].exchange_density(self.comm, *preps[0])]


class _LocalOps:
    """The same collectives over P jobs in one process (emulate_*)."""

    def reduce(self, tensors, op: str):
        torch = __import__("torch")
        stack = torch.stack([t.to(tensors[0].device) for t in tensors])
        red = {"sum": stack.sum(dim=0), "min": stack.amin(dim=0), "max": stack.amax(dim=0)}[op]
        return [red.to(dtype=t.dtype, device=t.device) for t in tensors]

    def gather_rows(self, tensors):
        torch = __import__("torch")
        return [torch.cat([t.to(u.device) for t in tensors]) for u in tensors]

    all_gather = gather_rows  # (equal shapes: the same concatenation)

    def gather_row(self, rows):
        torch = __import__("torch")
        return [torch.stack([t.to(u.device) for t in rows]) for u in rows]

    def exchange_density(self, sels, preps):
        u_fulls = self.all_gather([p[0] for p in preps])
        for s, u in zip(sels, u_fulls):
            s.set_density(s.density_contribution(u))
        return list(zip(u_fulls, self.all_gather([p[1] for p in preps])))


def _select(sels, ops, unlabeled_idx, forest, k, mode, strategy, beta, sort_fn, density_mode):
    """select over the jobs ``sels`` (one rank's selector, or P emulated
    shards) with the collectives ``ops``: one (indices, scores) per job.  Every
    decision is taken from values that are the same on every rank."""
    _soft_forest(forest, mode, strategy)
    unls = [s.index_tensor(unlabeled_idx) for s in sels]
    u_fulls = parts_fulls = [None] * len(sels)
    warm = [s._density is not None for s in sels]  # (a cold step's score kernel keeps the row-major pool)
    if mode in ALL_DENSITY_MODES:  # uncertainty sampling never normalises (no density, no zero-norm check)
        need_u = density_mode == "gram" and not all(warm)
        if need_u or any(s._parts_full is None for s in sels):
            preps = [s.prep() for s in sels]
            if need_u:  # the (small) canonical partials travel with the operand, beside the Gram
                u_fulls, parts_fulls = zip(*ops.exchange_density(sels, preps))
            else:
                parts_fulls = ops.all_gather([p[1] for p in preps])
            for s, parts in zip(sels, parts_fulls):
                s._parts_full = parts
                s._colsum = None  # derived from the partials, as the plans' captured column sum
                s._plans = {}
        parts_fulls = [s._parts_full for s in sels]
    all_valid = int(unls[0].shape[0]) >= k  # single source of truth for the candidate count

    def planned(s, u_full, unl):
        st = getattr(s, "state", None)  # (the CPU tests' oracle shards have none)
        return (st is not None and u_full is None and s._density is not None and s.world * k <= _lib.DAL_SORT_CAP
                and st.use_graphs and st.events_off() and st.n >= k and unl.is_cuda)

    if (mode == "dw" and density_mode == "gram" and sort_fn is hip_sort_positions
            and all(planned(s, u, unl) for s, u, unl in zip(sels, u_fulls, unls))):
        # warm step (density cached): the local step is one plan replay whose
        # outputs ARE the packed all-gather row; no host wait before the merge
        plans = [s.warm_plan(forest, k, beta) for s in sels]
        for plan, unl in zip(plans, unls):
            plan.launch(forest, unl)
        merged = [_merge_rows(g, k, all_valid) for g in ops.gather_row([plan.packed for plan in plans])]
    else:
        tops = [s.local_select(u, parts, unl, forest, k, mode, strategy, beta, density_mode, warm=w)
                for s, u, parts, unl, w in zip(sels, u_fulls, parts_fulls, unls, warm)]
        # every rank's status word (zero-norm rows, re-rank capacity overflow)
        # rides in the top-k all-gather and is read once, after the merge is
        # queued: the step's one host sync, and every rank sees the same bits
        merged = _merge(ops, tops, [s.status_word() for s in sels], sels[0].world, k, sort_fn, all_valid)
    st = merged[0][1]  # the OR of every rank's status word: identical on all ranks and jobs
    if mode not in ALL_DENSITY_MODES:
        st &= ~_lib.DAL_FLAG_ZERO_NORM  # a zero row only matters to the cosine density
    if st & _lib.DAL_FLAG_ZERO_NORM:
        raise ValueError("pool contains a zero-norm row: cosine similarity is undefined "
                         "(the reference would propagate NaN into every density)")
    if st & (_lib.DAL_FLAG_CAND_OVERFLOW | _lib.DAL_FLAG_SAMPLE_MISS):  # rare: redo on every rank
        for s in sels:
            s.prepare_retry(sample_miss=bool(st & _lib.DAL_FLAG_SAMPLE_MISS))
        return _select(sels, ops, unlabeled_idx, forest, k, mode, strategy, beta, sort_fn, density_mode)
    return [out for out, _ in merged]


def select(sel: ShardedSelector, comm, unlabeled_idx, forest, k: int, mode: str = "dw",
           strategy: str = "least_confidence", beta: float = 1.0, sort_fn=hip_sort_positions,
           density_mode: str = "gram"):
    """One selection step across all ranks; returns (indices [k], scores [k]),
    identical on every rank."""
    return _select([sel], _GroupOps(comm), unlabeled_idx, forest, k, mode, strategy, beta, sort_fn, density_mode)[0]


def emulate(selectors, unlabeled_idx, forest, k: int, mode: str = "dw",
            strategy: str = "least_confidence", beta: float = 1.0, sort_fn=hip_sort_positions,
            density_mode: str = "gram"):
    """select with P shards in one process (tests).  The P jobs must agree;
    their one (indices, scores) is returned."""
    return _same_topk(_select(list(selectors), _LocalOps(), unlabeled_idx, forest, k, mode, strategy, beta, sort_fn,
                              density_mode))


def _agreed(results, fingerprint, what: str):
    """emulate_*: the one result of P jobs, whose fingerprints must agree."""
    first = fingerprint(results[0])
    if any(fingerprint(r) != first for r in results[1:]):
        raise RuntimeError(f"the shards' {what} differ")
    return results[0]


def _same_topk(outs):
    """emulate, emulate_lal: every job must have merged the same (indices, score bits)."""
    return _agreed(outs, lambda o: [t.cpu().numpy().tobytes() for t in o], "merged selections")


def _pack_topk(top: LocalTopk, status=None):
    """A rank's (key, index, score) triples as one int64 row [3k] (scores by
    bit pattern), plus its status word when given ([3k + 1])."""
    torch = __import__("torch")
    parts = [top.keys, top.idx, top.scores.view(torch.int64)]
    if status is not None:
        parts.append(status.reshape(1).to(torch.int64))
    return torch.cat(parts)


def _unpack_topk(g, k: int):
    """Gathered rows [P, 3k (+1)] -> (keys, idx, scores) rank-major [P*k] (+ statuses [P])."""
    torch = __import__("torch")
    out = (g[:, :k].reshape(-1), g[:, k:2 * k].reshape(-1),
           g[:, 2 * k:3 * k].reshape(-1).contiguous().view(torch.float64))
    return out + (g[:, 3 * k],) if int(g.shape[1]) > 3 * k else out


def gather_topk(comm, top: LocalTopk, status=None):
    """ONE all-gather of every rank's packed row (_pack_topk): a collective's
    latency, not its bytes, dominates at k = 100-1000.
    Returns (keys, idx, scores) rank-major [P*k] (+ statuses [P])."""
    row = _pack_topk(top, status)
    w = int(row.shape[0])
    return _unpack_topk(comm.all_gather(row.reshape(1, w)).reshape(-1, w), int(top.keys.shape[0]))


def _merge(ops, tops, statuses, world: int, k: int, sort_fn, all_valid: bool, want_status: bool = True):
    """The merge of every rank's local top-k, per job: [((indices, scores), OR
    of the status words)].  ONE all-gather of the packed rows [3k + 1], then
    dal_topk_merge (_merge_rows) where the HIP sort takes world * k keys, else
    merge_topk with ``sort_fn`` and the statuses OR-ed on the host
    (want_status False: not read there, 0)."""
    gathered = ops.gather_row([_pack_topk(top, status) for top, status in zip(tops, statuses)])
    if sort_fn is hip_sort_positions and world * k <= _lib.DAL_SORT_CAP and tops[0].keys.is_cuda:
        return [_merge_rows(g, k, all_valid) for g in gathered]
    merged = []
    for g in gathered:
        keys_all, idx_all, sc_all, st_all = _unpack_topk(g, k)
        st = 0
        for v in (st_all.tolist() if want_status else ()):
            st |= int(v)
        merged.append((merge_topk(keys_all, idx_all, sc_all, k, sort_fn, all_valid=all_valid), st))
    return merged


def merge_packed(comm, top: LocalTopk, status, k: int, all_valid: bool = False):
    """gather_topk + merge_topk in one all-gather and one C call
    (dal_topk_merge reads the gathered [P, 3k+1] rows in place: unpack, sort
    by (key, rank-major position), gather; the status words OR-ed on the
    device).  Returns ((indices, scores), status) -- the status read is the
    step's one host sync."""
    return merge_row(comm, _pack_topk(top, status), k, all_valid)


def merge_row(comm, packed, k: int, all_valid: bool = False):
    """All-gather this rank's packed row int64 [3k+1] (keys | indices | score
    bits | status) and merge the rows with dal_topk_merge; returns ((indices,
    scores), OR of the status words)."""
    return _merge_rows(_GroupOps(comm).gather_row([packed])[0], k, all_valid)


def _merge_rows(g, k: int, all_valid: bool = False):
    """dal_topk_merge over the gathered packed rows [P, 3k+1]."""
    torch = __import__("torch")
    from .engine import _ptr, _stream
    from ._lib import call

    dev = g.device
    n_ranks, w = int(g.shape[0]), int(g.shape[1])
    lib = _lib.load()
    wsb = int(lib.dal_topk_merge_workspace_bytes(n_ranks, k))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None  # (the one-launch merge needs none)
    # the outputs in one allocation: indices | score bits | (keys) | status
    nk = 2 if all_valid else 3
    buf = torch.empty(nk * k + 1, dtype=torch.int64, device=dev)
    b0 = buf.data_ptr()
    call("dal_topk_merge", _ptr(g), n_ranks, w, k, 0 if ws is None else _ptr(ws), wsb, b0, b0 + 8 * k,
         0 if all_valid else b0 + 16 * k, b0 + 8 * nk * k, _stream(dev))
    st = int(buf[nk * k].item()) & 0xFFFFFFFF  # the int32 status in the low half (little endian)
    st = st - (1 << 32) if st >= (1 << 31) else st
    out_idx, out_sc = buf[:k], buf[k:2 * k].view(torch.float64)
    out_keys = None if all_valid else buf[2 * k:3 * k]
    if out_keys is not None:
        valid = out_keys != _as_i64(DAL_KEY_NONE)
        out_idx, out_sc = out_idx[valid], out_sc[valid]
    return (out_idx, out_sc), st


def _exclude_chunks(st, rows):
    """The rows of ``rows`` new to E (identical on every rank: E is global),
    in chunks one downdate takes."""
    new = st.new_excluded(rows)
    m = _lib.DAL_DOWNDATE_MAX_ROWS
    return new, [new[c0:c0 + m] for c0 in range(0, int(new.size), m)]


def _sum_delta(blocks, world: int):
    """Rank-major [P * m_pad, 2 * d_pad] int16 blocks -> their integer sum:
    exactly one rank owns each row of Delta and the others hold zeros, so the
    sum of the bit patterns (two halves per int32 lane: no carry can cross)
    reconstructs Delta exactly."""
    torch = __import__("torch")
    w = int(blocks.shape[1])
    return blocks.contiguous().view(torch.int32).reshape(world, -1, w // 2).sum(0, dtype=torch.int32) \
        .contiguous().view(torch.int16)


def _exclude_cold(sel: ShardedSelector, new):
    """No cached density (or gram "f32"): E u rows the invalidating way."""
    sel.state.set_excluded(np.union1d(sel.state.excluded, new))
    sel._density = None
    sel._parts_full = None
    sel._colsum = None
    sel._plans = {}


def _exclude(sels, ops, rows) -> int:
    """exclude over the jobs ``sels`` with the collectives ``ops``; the count
    of newly excluded rows (E is global: one number for every job)."""
    new, chunks = _exclude_chunks(sels[0].state, rows)
    if new.size == 0:
        return 0
    if any(s._density is None for s in sels) or sels[0].state.gram == "f32":
        for s in sels:
            _exclude_cold(s, new)
        return int(new.size)
    for chunk in chunks:
        for s, blocks in zip(sels, ops.all_gather([s.state.delta_operand(chunk) for s in sels])):
            s.state.apply_exclude(chunk, _sum_delta(blocks, s.world))
    for s, parts in zip(sels, ops.all_gather([s.prep()[1] for s in sels])):
        s._parts_full = parts
        s._colsum = None
        s._plans = {}
    return int(new.size)


def exclude(sel: ShardedSelector, comm, rows) -> int:
    """PoolState.exclude across all ranks (every rank calls it with the same
    ``rows``, global indices): one small all-gather per chunk carries the
    operand rows of Delta -- each rank contributes the rows it owns, zeros
    elsewhere --, every rank lowers its own density slice by their cosine sums
    and repairs its own flags, operand and partials; the partials are
    all-gathered again and the global column sum and the warm plans are
    rebuilt on the next step.  Ranks that own none of Delta, and empty
    shards, take part in the collectives and leave their rows as they are.
    Returns the count of newly excluded rows."""
    return _exclude([sel], _GroupOps(comm), rows)


def emulate_exclude(selectors, rows) -> int:
    """exclude with P shards in one process (tests)."""
    return _exclude(list(selectors), _LocalOps(), rows) if selectors else 0


def diversity_select_sharded(x_local, row_base: int, labeled_rows, k: int, comm, candidates=None,
                             device=None, sort_fn=hip_sort_positions):
    """Batch-mode diversity selection (BASELINE config 5) over a row-sharded
    bf16 pool: every rank scores its rows against the replicated labeled set
    (no exchange), keeps its exact local top-k, and the all-gathered lists are
    merged identically on every rank."""
    from .similarity import diversity_select

    n = int(x_local.shape[0])
    dev = x_local.device if device is None else device
    top = LocalTopk.empty(k, dev)
    if n:
        sel = diversity_select(x_local, None, k, candidates=candidates, device=dev, row_base=row_base,
                               labeled_rows=labeled_rows)
        kk = int(sel.indices.shape[0])
        top.idx[:kk] = sel.indices
        top.scores[:kk] = sel.selected_scores
        top.keys[:kk] = _score_keys_asc(sel.selected_scores)
    return merge_topk(*gather_topk(comm, top), k, sort_fn)


def _score_keys_asc(s):
    """Ascending score keys of finite fp64 scores, computed on the device with
    the C ABI's encoding (-0 -> +0; negative -> ~bits; else bits | sign bit),
    stored as int64 bit patterns of the uint64 keys."""
    torch = __import__("torch")
    s = torch.where(s == 0, torch.zeros_like(s), s)
    b = s.view(torch.int64)
    return torch.where(b < 0, ~b, b | (-(1 << 63)))


# ------------------------------------------------------------------ LAL --
def _lal_local_topk(sel: ShardedSelector, flags, votes, hist_global, forest, lal_model, k: int, n_labeled: int,
                    n_positive: int) -> LocalTopk:
    """A rank's LAL scores from the GLOBAL vote histogram (every rank computes
    the same T + 1 rows and the same LUT) and its exact local top-k."""
    from .engine import lal_scores, topk_keys

    st = sel.state
    out = LocalTopk.empty(k, st.device)
    if st.n == 0:
        return out
    _, sc, kys = lal_scores(st, forest, lal_model, flags, votes, hist_global, n_labeled, n_positive)
    kk = min(k, st.n)
    i, kk_keys = topk_keys(kys, kk, st.row_base)
    out.keys[:kk], out.idx[:kk], out.scores[:kk] = kk_keys, i, sc[i - st.row_base]
    return out


def _lal_local_votes(sel: ShardedSelector, unl, forest):
    """(flags, votes, local vote histogram int64 [T + 1]) of a rank's shard."""
    from .engine import lal_votes

    _soft_forest(forest, "lal")
    torch = __import__("torch")
    st = sel.state
    if st.n == 0:
        return None, None, torch.zeros(forest.n_trees + 1, dtype=torch.int64, device=st.device)
    flags, _, _ = st.row_flags(unl)
    votes, hist = lal_votes(st, forest, flags)
    return flags, votes, hist


def _select_lal(sels, ops, unlabeled_idx, forest, lal_model, k, n_labeled, n_positive, sort_fn):
    """select_lal over the jobs ``sels`` with the collectives ``ops``: one
    (indices, scores) per job."""
    from .engine import check_lal_inputs

    check_lal_inputs(forest, lal_model, n_labeled, n_positive)
    unls = [s.index_tensor(unlabeled_idx) for s in sels]
    n_unl_global = int(unls[0].shape[0])
    if n_unl_global == 0:
        raise ValueError("unlabeled set is empty (the reference loop breaks here)")
    local = [_lal_local_votes(s, unl, forest) for s, unl in zip(sels, unls)]
    hists = ops.reduce([hist for _, _, hist in local], "sum")
    tops = [_lal_local_topk(s, flags, votes, hist, forest, lal_model, k, n_labeled, n_positive)
            for s, (flags, votes, _), hist in zip(sels, local, hists)]
    # (the status word rides in the packed row and is not acted on: nothing here sets it)
    merged = _merge(ops, tops, [s.status_word() for s in sels], sels[0].world, k, sort_fn,
                    all_valid=n_unl_global >= k, want_status=False)
    return [out for out, _ in merged]


def select_lal(sel: ShardedSelector, comm, unlabeled_idx, forest, lal_model, k: int, n_labeled: int,
               n_positive: int, sort_fn=hip_sort_positions):
    """One LAL selection step across all ranks (dal.active_learner.select_lal
    row-sharded); returns (indices [k], scores [k]), identical on every rank
    and for every P.  Each rank takes its shard's votes and vote histogram;
    the histograms are summed by ONE all_reduce of T + 1 int64 (integers: the
    same bits in any order); every rank then builds the same rows and LUT,
    rescores its rows and keeps its local top-k, merged as mode "us" does."""
    return _select_lal([sel], _GroupOps(comm), unlabeled_idx, forest, lal_model, k, n_labeled, n_positive, sort_fn)[0]


def emulate_lal(selectors, unlabeled_idx, forest, lal_model, k: int, n_labeled: int, n_positive: int,
                sort_fn=hip_sort_positions):
    """select_lal with P shards in one process (tests).  The P jobs must
    agree; their one (indices, scores) is returned."""
    return _same_topk(_select_lal(list(selectors), _LocalOps(), unlabeled_idx, forest, lal_model, k, n_labeled,
                                  n_positive, sort_fn))


# --------------------------------------------------------- StandardScaler --
def _device_moments(x_local, fmt=None):
    """The local steps of fit_scaler on the GPU (dal.dataset): fmt None ->
    (low, top, nonfinite) of the shard; fmt = (q, k1, k2) -> its cells."""
    from . import dataset as ds

    torch = __import__("torch")
    x, n, d, ldx = ds._device_rows(x_local)
    if fmt is None:
        low, top, status = ds.device_format(x, n, d, ldx)
        return low, top, (status & _lib.DAL_FLAG_NONFINITE).ne(0).to(torch.int32)
    q, k1, k2 = fmt
    return ds.device_accumulate(x, n, d, ldx, q, k1, k2)


def _scaler_model(cells_and_n, q, k1: int, k2: int, with_mean: bool, with_std: bool):
    """The host finish from the summed cells, the total row count in the last word."""
    from . import dataset as ds

    buf = cells_and_n.cpu().numpy()
    n = int(buf[-1])
    if n > ds.MAX_ROWS:
        raise ValueError(f"{n} rows in total: the exact sums take at most {ds.MAX_ROWS}")
    mean, std = ds.moments_from_cells(buf[:-1], q, k1, k2, n)
    return ds.StandardScalerModel(mean, std, n, with_mean, with_std)


def _cells_and_rows(cells, n_local: int):
    torch = __import__("torch")
    return torch.cat([cells.reshape(-1), torch.tensor([n_local], dtype=torch.int64, device=cells.device)])


def _fit_scaler(shards, ops, accumulate_fn, with_mean: bool, with_std: bool):
    """fit_scaler over the jobs ``shards`` with the collectives ``ops``: one
    StandardScalerModel per job."""
    from . import dataset as ds

    torch = __import__("torch")
    fn = accumulate_fn or _device_moments
    lows, his = [], []
    for x_local in shards:
        low, top, bad = fn(x_local, None)
        lows.append(low.clone())
        his.append(torch.cat([top.reshape(-1), torch.as_tensor(bad, dtype=torch.int32, device=top.device).reshape(1)]))
    low = ops.reduce(lows, "min")[0]
    hi = ops.reduce(his, "max")[0].cpu().numpy()  # the columns' tops, then any rank's non-finite flag
    k1, k2, q = ds.check_format(low.cpu().numpy(), hi[:-1], int(hi[-1]))
    bufs = ops.reduce([_cells_and_rows(fn(x_local, (q, k1, k2)), int(x_local.shape[0])) for x_local in shards], "sum")
    return [_scaler_model(buf, q, k1, k2, with_mean, with_std) for buf in bufs]


def fit_scaler(x_local, comm, accumulate_fn=None, with_mean: bool = True, with_std: bool = True):
    """dal.dataset.StandardScaler.fit over row shards: the same mean and std
    bytes on every rank and for every P.  All-reduce MIN of the columns' lowest
    set bits and MAX of their tops (int32, with the non-finite flag), the local
    accumulate, ONE all-reduce SUM of the int64 cells (with the row count),
    then every rank finishes alike.  An empty shard [0, d] is legal.
    accumulate_fn(x_local, fmt): the two local steps (tests inject the
    restatement; None: the HIP kernels) -- fmt None returns (low, top,
    nonfinite flag), fmt = (q, k1, k2) returns the shard's cells [d, k1 + k2]."""
    return _fit_scaler([x_local], _GroupOps(comm), accumulate_fn, with_mean, with_std)[0]


def emulate_fit_scaler(shards, accumulate_fn=None, with_mean: bool = True, with_std: bool = True):
    """fit_scaler with P shards in one process (tests).  The P jobs must
    agree; their one model is returned."""
    models = _fit_scaler(list(shards), _LocalOps(), accumulate_fn, with_mean, with_std)
    return _agreed(models, lambda m: (m.mean.tobytes(), m.std.tobytes(), m.n), "scaler fits")


# ------------------------------------------------------------ evaluation --
def _device_table(x_local, y_local, forest):
    """The local step of evaluate on the GPU: the shard's joint table
    (dal.metrics.joint_histogram), a device int64 tensor."""
    from . import metrics
    from .engine import PoolState

    torch = __import__("torch")
    state = x_local if isinstance(x_local, PoolState) else PoolState(x_local)
    labels = torch.from_numpy(metrics.check_labels(y_local, state.n, forest)).to(state.device)
    return metrics.joint_histogram(forest, state, labels, build_blocked=isinstance(x_local, PoolState))


def _shard_table(fn, x_local, y_local, forest):
    """One shard's table as a flat int64 tensor of the table's size."""
    from . import metrics

    torch = __import__("torch")
    rows, cols = metrics.table_shape(forest.n_trees, forest.n_classes)
    t = torch.as_tensor(fn(x_local, y_local, forest)).to(torch.int64).reshape(-1)
    if t.numel() != rows * cols:
        raise ValueError(f"a shard's table holds {t.numel()} cells, not {rows * cols}")
    return t


def _evaluate(shards, forest, ops, hist_fn, measures):
    """evaluate over the jobs ``shards`` = [(x_local, y_local)] with the
    collectives ``ops``: one dict per job."""
    from . import metrics

    names = metrics.check_measures(measures, forest.n_classes)
    fn = hist_fn or _device_table
    bufs = ops.reduce([_shard_table(fn, x, y, forest).clone() for x, y in shards], "sum")
    return [metrics.finish(buf.cpu().numpy(), forest.n_trees, forest.n_classes, names) for buf in bufs]


def evaluate(x_local, y_local, forest, comm, hist_fn=None, measures=("accuracy",)):
    """dal.metrics.evaluate over row shards: every rank computes its shard's
    joint table, ONE all_reduce SUM of the int64 cells, then every rank
    finishes alike -- the dict is the same bytes on every rank and for every
    P (integers: the sum does not depend on the order).  An empty shard
    [0, d] is legal.  hist_fn(x_local, y_local, forest) -> table: the local
    step (tests inject the restatement; None: the HIP kernel, with x_local an
    array or a PoolState)."""
    return _evaluate([(x_local, y_local)], forest, _GroupOps(comm), hist_fn, measures)[0]


def emulate_evaluate(shards, forest, hist_fn=None, measures=("accuracy",)):
    """evaluate with P shards [(x, y), ...] in one process (tests).  The P
    jobs must agree; their one dict is returned."""
    dicts = _evaluate(list(shards), forest, _LocalOps(), hist_fn, measures)
    return _agreed(dicts, lambda d: [(name, np.asarray(v).tobytes()) for name, v in sorted(d.items())], "measures")


# --------------------------------------------------------- forest training --
def _sharded_fit(regress: bool, shards, n_total: int, ops, steps, num_trees, max_depth, max_bins, seed,
                 feature_subset_strategy, weights, feature_subsets, min_instances_per_node, min_info_gain,
                 num_classes=2, tree_chunk=None):
    """train_classifier / train_regressor over the jobs of ``shards`` =
    [(x_local, y_local, positions)] with the local halves ``steps`` (one per
    job) and the collectives ``ops``.  Every decision below is taken from
    values that are the same on every rank, so the ranks raise or proceed
    alike."""
    from types import SimpleNamespace

    from . import random_forest as rf

    torch = __import__("torch")
    n_total, P = int(n_total), len(shards)
    if n_total < 1:
        raise ValueError("training set must be non-empty")
    # -- local checks: a failure is kept and raised after the first collective, on every rank
    xs, ys, poss, bounds, cover, meta, errors = [], [], [], [], [], [], []
    for (x_local, y_local, positions), st in zip(shards, steps):
        x = pos = y = bound = None
        seen = np.zeros(n_total, dtype=np.int64)
        d = f64 = 0
        try:
            x = st.rows(x_local, regress)
            yv = y_local.cpu().numpy() if isinstance(y_local, torch.Tensor) else np.asarray(y_local)
            pos = (positions.cpu().numpy() if isinstance(positions, torch.Tensor) else np.asarray(positions))
            pos = pos.astype(np.int64).reshape(-1)
            if x.dim() != 2 or x.shape[1] < 1:
                raise ValueError("a shard must be a 2-D [rows, features] array (an empty one [0, d])")
            n_local, d, f64 = int(x.shape[0]), int(x.shape[1]), int(x.dtype == torch.float64)
            if pos.shape[0] != n_local or (n_local and (pos.min() < 0 or pos.max() >= n_total)):
                raise ValueError(f"positions must be {n_local} indices in [0, {n_total}), one per local row")
            seen[:] = np.bincount(pos, minlength=n_total)
            if regress:
                y, b_y, b_sq = rf.regression_label_bounds(yv, n_local)
                bound = (b_y[0], b_sq[0], -b_y[1], -b_sq[1])
            else:
                y = rf.check_labels(yv, n_local, num_classes)
        except ValueError as e:
            errors.append(e)
        xs.append(x), ys.append(y), poss.append(pos), bounds.append(bound), cover.append(seen)
        meta.append([d, -d, f64, -f64, int(len(errors) > len(meta))])
    devs = [x.device if x is not None else getattr(st, "dev", torch.device("cpu")) for x, st in zip(xs, steps)]
    # one all-reduce MAX: any rank's refusal, and the feature count and row dtype every rank must share
    d, nd, f64, nf64, refused = ops.reduce([torch.tensor(m, dtype=torch.int64, device=dv)
                                            for m, dv in zip(meta, devs)], "max")[0].cpu().tolist()
    if errors:
        raise errors[0]
    if refused:
        raise ValueError("another rank's rows, labels or positions were refused")
    if d != -nd:
        raise ValueError(f"the ranks' shards must have one feature count: they range from {-nd} to {d}")
    if f64 != -nf64:
        raise ValueError("the ranks' rows must have one dtype (fp32, or fp64), empty shards included")
    seen = ops.reduce([torch.from_numpy(c).to(dv) for c, dv in zip(cover, devs)], "sum")[0].cpu().numpy()
    if (seen != 1).any():
        bad = int(np.nonzero(seen != 1)[0][0])
        raise ValueError(f"positions must cover [0, {n_total}) exactly once over the ranks: position {bad} "
                         f"appears {int(seen[bad])} times")
    # -- the global host inputs (the single-device fit's, over n_total rows), the same on every rank
    rf.check_growth(max_depth, max_bins)
    if regress:
        lim = [torch.tensor(b, dtype=torch.int64, device=dv) for b, dv in zip(bounds, devs)]
        low_y, low_sq, ntop_y, ntop_sq = (int(v) for v in ops.reduce(lim, "min")[0].cpu().tolist())
        (q_y, k_y), (q_sq, k_sq) = rf.regression_formats((low_y, -ntop_y), (low_sq, -ntop_sq))
        g = rf.regressor_inputs(n_total, d, num_trees, max_depth, max_bins, seed, feature_subset_strategy, weights,
                                feature_subsets, k_y, k_sq)
        rows = rf.regression_split_sample_rows(n_total, max_bins, seed, bool(f64))
        chunk = rf.regressor_tree_chunk(tree_chunk, n_total, g.T, max_depth, g.m, g.ns, k_y, k_sq)
        fmt = (q_y, k_y, q_sq, k_sq)
    else:
        g = rf.classifier_inputs(n_total, d, None, 0, num_trees, max_depth, max_bins, seed, feature_subset_strategy,
                                 weights, feature_subsets, num_classes, check_weights=True)
        rows, chunk, fmt = g.rows, g.T, None
    # -- thresholds: the sample's rows from wherever they live, the same search on every rank
    picks = [x if rows is None else x[torch.from_numpy(np.nonzero(np.isin(pos, rows))[0]).to(x.device)]
             for x, pos in zip(xs, poss)]
    found = [st.find_splits(s, g.ns, regress) for st, s in zip(steps, ops.gather_rows(picks))]
    # -- levels: statistics, ONE all-reduce SUM, split; no host read
    caches = [{} for _ in range(P)]
    outs = [[] for _ in range(P)]
    for t0 in range(0, g.T, chunk):
        t1 = min(g.T, t0 + chunk)
        for i, st in enumerate(steps):
            st.begin(SimpleNamespace(
                regress=regress, x=xs[i], y=ys[i], weights=np.ascontiguousarray(g.weights[t0:t1][:, poss[i]]),
                subsets=g.subsets[t0:t1], thresholds=found[i][0], n_splits=found[i][1], ns=g.ns, m=g.m,
                max_depth=max_depth, min_instances=int(min_instances_per_node), min_gain=float(min_info_gain),
                num_classes=int(num_classes), fmt=fmt, cache=caches[i]))
        for level in range(max_depth + 1):
            reduced = ops.reduce([st.level_stats(level) for st in steps], "sum")
            for st, r in zip(steps, reduced):
                st.split(level, r)
        for i, st in enumerate(steps):
            outs[i].append(st.finish())
    flags = ops.reduce([torch.as_tensor(f[2]).reshape(1).to(torch.int32) for f in found], "max")
    rf.check_split_overflow(flags[0].item())
    models = []
    for i in range(P):
        arrays = [torch.cat(a) if isinstance(a[0], torch.Tensor) else np.concatenate(a) for a in zip(*outs[i])]
        models.append(rf.regression_forest(*arrays, max_depth, found[i][0], found[i][1]) if regress else
                      rf.classifier_forest(*arrays, max_depth, num_classes, found[i][0], found[i][1]))
    return models


def _same_model(models, regress: bool):
    """emulate_*: every job must have grown the same forest."""
    names = ("inner_feature", "inner_threshold", "leaf") if regress else ("inner", "leaf")
    return _agreed(models, lambda m: [getattr(m, a).tobytes() for a in names], "fits")


def train_classifier(x_local, y_local, positions, n_total: int, comm, num_trees: int = 10, max_depth: int = 4,
                     max_bins: int = 32, seed: int = 0, feature_subset_strategy: str = "auto", weights=None,
                     feature_subsets=None, min_instances_per_node: int = 1, min_info_gain: float = 0.0,
                     num_classes: int = 2, steps=None):
    """dal.random_forest.train_classifier over row shards: on every rank the
    same Forest bytes as the single-device fit of the n_total rows in
    canonical order, for every number of ranks and every assignment of rows
    to ranks (MLlib's own distribution: per-partition level aggregates,
    summed, one split decision).

    x_local [n_local, d] and y_local [n_local] are the rank's rows (an empty
    shard [0, d] is legal); positions int64 [n_local] are their indices in the
    canonical training set [0, n_total) -- contiguous shards and scattered
    labeled rows alike.  Over the ranks the positions must cover [0, n_total)
    exactly once: checked with one all-reduce SUM of the per-position counts,
    after one all-reduce MAX that carries any rank's local refusal and the
    feature count and row dtype the ranks must share; ValueError on every
    rank alike otherwise.  ``weights`` [T, n_total] /
    ``feature_subsets`` are the global draws (default: bagging_inputs over
    n_total on every rank -- the host draw of the single-device fit); a rank
    uses the columns ``positions``.  Every tree's global weight sum must stay
    below 2^31 (check_tree_weights).  The thresholds are searched on every
    rank over the all-gathered split sample (counts, then rows padded to the
    largest count); numSplits is that of n_total.  Per level: the local
    statistics, ONE all-reduce SUM of the level's int32 span, the split -- all
    stream-ordered, no host read; then the threshold-overflow flag is
    MAX-reduced and read once.

    steps: the local half (dal.random_forest.HipSteps documents the methods;
    None: the HIP entries on the current device; tests inject a restatement)."""
    from .random_forest import HipSteps

    return _sharded_fit(False, [(x_local, y_local, positions)], n_total, _GroupOps(comm), [steps or HipSteps()],
                        num_trees, max_depth, max_bins, seed, feature_subset_strategy, weights, feature_subsets,
                        min_instances_per_node, min_info_gain, num_classes=num_classes)[0]


def train_regressor(x_local, y_local, positions, n_total: int, comm, num_trees: int = 10, max_depth: int = 4,
                    max_bins: int = 32, seed: int = 0, feature_subset_strategy: str = "auto", weights=None,
                    feature_subsets=None, min_instances_per_node: int = 1, min_info_gain: float = 0.0,
                    tree_chunk=None, steps=None):
    """dal.random_forest.train_regressor over row shards, as train_classifier
    above: the same RegressionForest bytes on every rank, for every sharding
    and every ``tree_chunk`` (the chunk loop stays outside the level loop; the
    default chunk is sized from n_total, so the ranks agree on it).  The exact
    sums' formats (q, k) of y and fl(y * y) come from an all-reduce MIN of the
    shards' lowest set bits and negated tops; an empty or all-zero shard
    contributes no value.  A non-finite label anywhere raises ValueError on
    every rank.  Every rank's rows have one dtype (fp32, or fp64 for unrounded
    rows), empty shards included.  ONE all-reduce SUM of int64 words per level."""
    from .random_forest import HipSteps

    return _sharded_fit(True, [(x_local, y_local, positions)], n_total, _GroupOps(comm), [steps or HipSteps()],
                        num_trees, max_depth, max_bins, seed, feature_subset_strategy, weights, feature_subsets,
                        min_instances_per_node, min_info_gain, tree_chunk=tree_chunk)[0]


def _emulate_steps(steps, P: int):
    from .random_forest import HipSteps

    return [(steps or HipSteps)() for _ in range(P)]


def emulate_train_classifier(shards, n_total: int, num_trees: int = 10, max_depth: int = 4, max_bins: int = 32,
                             seed: int = 0, feature_subset_strategy: str = "auto", weights=None,
                             feature_subsets=None, min_instances_per_node: int = 1, min_info_gain: float = 0.0,
                             num_classes: int = 2, steps=None):
    """train_classifier with P shards [(x, y, positions), ...] in one process
    (tests): each all-reduce becomes an elementwise sum / min / max over the
    shards, the all-gather a concatenation.  steps: a zero-argument factory of
    the local half, called once per shard (None: HipSteps).  The P jobs must
    agree; their one Forest is returned."""
    models = _sharded_fit(False, list(shards), n_total, _LocalOps(), _emulate_steps(steps, len(shards)), num_trees,
                          max_depth, max_bins, seed, feature_subset_strategy, weights, feature_subsets,
                          min_instances_per_node, min_info_gain, num_classes=num_classes)
    return _same_model(models, False)


def emulate_train_regressor(shards, n_total: int, num_trees: int = 10, max_depth: int = 4, max_bins: int = 32,
                            seed: int = 0, feature_subset_strategy: str = "auto", weights=None,
                            feature_subsets=None, min_instances_per_node: int = 1, min_info_gain: float = 0.0,
                            tree_chunk=None, steps=None):
    """train_regressor with P shards in one process, as emulate_train_classifier."""
    models = _sharded_fit(True, list(shards), n_total, _LocalOps(), _emulate_steps(steps, len(shards)), num_trees,
                          max_depth, max_bins, seed, feature_subset_strategy, weights, feature_subsets,
                          min_instances_per_node, min_info_gain, tree_chunk=tree_chunk)
    return _same_model(models, True)


# ------------------------------------------------------- greedy k-center --
def _kcenter(shards, ops, steps, labeled_rows, k: int, candidates, weights=None, alpha=None):
    """kcenter_select_sharded over the jobs of ``shards`` = [(x_local,
    row_base)] with the local halves ``steps`` (one per job) and the
    collectives ``ops``: one all-reduce SUM of the in-range candidate counts
    fixes the number of steps on every rank alike; then per step propose, one
    all-gather of one record per rank, commit -- no host read in the loop.

    weights: one fp64 array per job (the shard's rows) makes it the ranked
    batch-mode selection; its default alpha is formed from the all-reduced
    count, the same float on every rank."""
    from .engine import Selection

    if int(k) < 1:
        raise ValueError("k must be >= 1")
    if weights is None:
        counts = [st.prepare(x_local, row_base, labeled_rows, candidates)
                  for (x_local, row_base), st in zip(shards, steps)]
    else:
        from .similarity import check_alpha, default_alpha

        if alpha is not None:
            alpha = check_alpha(alpha)
        counts = [st.prepare(x_local, row_base, labeled_rows, candidates, weights=w, alpha=alpha)
                  for (x_local, row_base), st, w in zip(shards, steps, weights)]
    total = int(ops.reduce(counts, "sum")[0].item())
    kk = min(int(k), total)
    if weights is not None and alpha is None:
        for st in steps:
            st.alpha = default_alpha(total, len(labeled_rows))
    for st in steps:
        st.begin(kk)
    for t in range(kk):
        for st, records in zip(steps, ops.gather_row([st.propose(t) for st in steps])):
            st.commit(t, records)
    sels = []
    for st in steps:
        idx, sc, scores = st.finish()
        sel = Selection(scores=scores, indices=idx, selected_scores=sc)
        if weights is not None:
            sel.selected_similarity = st.selected_similarity
        sels.append(sel)
    return sels


def kcenter_select_sharded(x_local, row_base: int, labeled_rows, k: int, comm, candidates=None, device=None,
                           steps=None):
    """dal.similarity.kcenter_select over a row-sharded bf16 pool: on every
    rank the indices and fp64 pick-time values of the single-device selection
    of the whole pool, for every shard count, uneven and empty shards included.

    x_local [n_local, d] are the rank's rows (global index of row 0:
    ``row_base``), ``labeled_rows`` [m, d] the labeled set replicated on every
    rank, ``candidates`` global indices (None: every row of every shard).  One
    all-reduce SUM of the in-range candidate counts up front fixes the number
    of steps; per step: the rank's best row (dal_kcenter_propose), ONE
    all-gather of one record per rank (TorchComm.all_gather_rows), the pick and
    the update pass (dal_kcenter_commit) -- stream-ordered, no host read inside
    the loop.  ``scores`` are the fp32 max-cosines of the rank's own
    candidates after the last pick.

    steps: the local half (dal.similarity.HipKCenterSteps documents the
    methods; None: the HIP entries on ``device``; tests inject a restatement)."""
    from .similarity import HipKCenterSteps

    return _kcenter([(x_local, row_base)], _GroupOps(comm), [steps or HipKCenterSteps(device)], labeled_rows, k,
                    candidates)[0]


def emulate_kcenter(shards, labeled_rows, k: int, candidates=None, steps=None):
    """kcenter_select_sharded with P shards [(x_local, row_base), ...] in one
    process (tests): the all-reduce becomes a sum over the shards, the
    all-gather a stack.  steps: a zero-argument factory of the local half,
    called once per shard (None: HipKCenterSteps).  The P jobs must agree on
    the picks; the Selection carries them and the shards' scores concatenated
    in shard order."""
    from .similarity import HipKCenterSteps

    shards = list(shards)
    sels = _kcenter(shards, _LocalOps(), [(steps or HipKCenterSteps)() for _ in shards], labeled_rows, k, candidates)
    return _same_selection(sels)


def _same_selection(sels):
    """The one Selection of P emulated jobs, which must agree on the picks: it
    carries them and the shards' scores concatenated in shard order."""
    from .engine import Selection

    torch = __import__("torch")
    ranked = hasattr(sels[0], "selected_similarity")
    picks = ("indices", "selected_scores") + (("selected_similarity",) if ranked else ())
    first = _agreed(sels, lambda s: [getattr(s, a).cpu().numpy().tobytes() for a in picks], "k-center selections")
    sel = Selection(scores=torch.cat([s.scores.to(first.scores.device) for s in sels]), indices=first.indices,
                    selected_scores=first.selected_scores)
    if ranked:
        sel.selected_similarity = first.selected_similarity
    return sel


def ranked_batch_select_sharded(x_local, row_base: int, labeled_rows, weights_local, k: int, comm, alpha=None,
                                candidates=None, device=None, steps=None):
    """dal.similarity.ranked_batch_select over a row-sharded bf16 pool, as
    kcenter_select_sharded: on every rank the indices, fp64 scores and
    ``selected_similarity`` of the single-device selection of the whole pool,
    for every shard count.  ``weights_local``: fp64, one per row of x_local.
    alpha None: |C| / (|C| + m) from the candidate count that the up-front
    all-reduce already sums, so every rank forms the same float; it is one
    number per call, not recomputed per pick.  Still ONE all-gather of one
    record per rank per step (the record's reserved word carries the pick's
    similarity)."""
    from .similarity import HipKCenterSteps

    return _kcenter([(x_local, row_base)], _GroupOps(comm), [steps or HipKCenterSteps(device)], labeled_rows, k,
                    candidates, weights=[weights_local], alpha=alpha)[0]


def emulate_ranked_batch(shards, labeled_rows, weights, k: int, alpha=None, candidates=None, steps=None):
    """ranked_batch_select_sharded with P shards [(x_local, row_base), ...] and
    their weights [w_local, ...] in one process (tests), as emulate_kcenter."""
    from .similarity import HipKCenterSteps

    shards = list(shards)
    sels = _kcenter(shards, _LocalOps(), [(steps or HipKCenterSteps)() for _ in shards], labeled_rows, k, candidates,
                    weights=list(weights), alpha=alpha)
    return _same_selection(sels)
