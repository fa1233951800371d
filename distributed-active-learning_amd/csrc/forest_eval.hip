// Test-set evaluation of a forest: the joint histogram of (vote, label) in one
// fused pass that stores nothing per row.
//
// Reference: lal_direct_mllib_implementation/classes/active_learner.py:95-121
// (ActiveLearner.evaluate: accuracy, TN / TP / FN / FP and the AUC of the test
// split) and the loop scripts' per-iteration test accuracy
// (final_thesis/uncertainty_sampling.py:80-82, :113).  Every one of those
// measures is a function of one small integer table:
//   n_classes == 2   hist[T + 1][2], cell [v][y]: rows with v trees voting 1
//                    and label y;
//   n_classes  > 2   hist[C][C], cell [y][pred]: pred the smallest class with
//                    the most trees (dal_forest_score_multiclass's pred).
// The host finishes each measure from the table in integers (dal.metrics).
//
// MI355X design.  The blocked kernel is forest_multi_blocked.hip's, as it is: a
// persistent grid, the prepared forest (dal_forest_prepare) copied into LDS
// once per block, per 64-row tile only the runs of the features the forest
// tests, staged by LDS-DMA (all NW waves issue), the rows on the 64 lanes of
// every wave and the trees dealt over the NW waves, byte-addressed walks
// (forest_shared.hpp), the waves' partial counts summed by wave 0 through an
// LDS exchange region.  Where the score kernels' epilogue writes 20 B per row,
// this one reads one label byte (and one flag byte) per row and adds 1 to a
// 32-bit counter of the block's table in LDS -- lal.hip's vote_histogram_kernel
// with its wave-uniform shortcut: a confident forest puts most rows of a tile
// into two cells, and per-lane LDS atomics on one address serialise.  When the
// block ends it issues one 64-bit global atomic per occupied cell: integer
// adds, exact in any order, so the table is the same words for every grid, row
// order and sharding.  The row-major kernel (no blocked copy, or a forest the
// blocked rule refuses) is one thread per row over x with the forest read from
// global memory, the same cells.
//
// LDS of the blocked kernel: [tile, fu_max runs of 256 B | prepared payload |
// table, round4(cells) u32 | exchange, NW - 1 waves' partial counts of the 64
// rows]: CW 32-bit words per row for C classes, one 16-bit word in the binary
// form (the sum of the leaf bytes, or bit 15 for a byte >= 2).
// (the header's out-of-line density power serves the score kernels only)
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "forest_shared.hpp"

namespace dal {
namespace {

constexpr int kEvIlp = 4;    // independent tree walks in flight per lane
constexpr int kEvPerCu = 5;  // blocks per CU at most (forest.hip, DAL_FOREST_BLOCKED_PER_CU)
constexpr int kEvWaves = 4;
constexpr int kEvWavesWide = 8;
constexpr int kEvRowThreads = 256;  // the row-major kernel's block

struct EvalArgs {
  int64_t n;
  int d;
  int n_trees;
  int depth;
  int n_classes;
  int n_cells;
  const uint8_t* labels;
  const uint8_t* flags;  // nullable: every row is counted
  unsigned long long* hist;
};

// One row's cell into the block's table, all 64 lanes of a wave together
// (cell < 0: the lane adds nothing).  A wave whose counted lanes all hold one
// cell adds its lane count once (vote_histogram_kernel's shortcut).
__device__ __forceinline__ void table_add(unsigned* s_hist, int cell, int lane) {
  const bool counted = cell >= 0;
  const unsigned long long mask = __ballot(counted);
  if (mask == 0ull) return;  // wave-uniform
  const int lead = __ffsll(static_cast<long long>(mask)) - 1;
  const int c0 = __shfl(cell, lead);
  if (__ballot(counted && cell == c0) == mask) {
    if (lane == lead) atomicAdd(&s_hist[c0], static_cast<unsigned>(__popcll(mask)));
  } else if (counted) {
    atomicAdd(&s_hist[cell], 1u);
  }
}

// The binary form walks as the score kernel does, one add per tree: the leaf
// bytes are summed (the vote count while every byte is 0 or 1) and, one more
// instruction, ORed (a byte >= 2 leaves a bit above bit 0).  A thread's word for
// its trees, 16 bits: the sum (<= T <= 4095), or bit 15 alone when a byte was
// >= 2; the words of a row's (at most 8) threads add without a carry into bit
// 15, so any bit from 15 up marks the row.
__device__ __forceinline__ unsigned binary_word(unsigned sum, unsigned any) { return any > 1u ? 32768u : sum; }
__device__ __forceinline__ int binary_cell(unsigned w, unsigned y) {
  return (w >> 15) == 0u && y < 2u ? static_cast<int>(2u * w + y) : -1;
}

// The C-class cell [y][pred] from a row's packed counts: pred the lowest class
// holding the largest count (row_epilogue's arg); a row one of whose trees
// ended in a leaf byte >= C (its counts sum to less than T) has no cell.
template <int CW>
__device__ __forceinline__ int multiclass_cell(const unsigned (&w)[CW], int C, int n_trees, unsigned y) {
  int m1 = -1, arg = 0, sum = 0;
#pragma unroll
  for (int c = 0; c < 4 * CW; ++c) {
    if (c < C) {
      const int nc = vote_field<CW>(w, c);
      sum += nc;
      if (nc > m1) {
        m1 = nc;
        arg = c;
      }
    }
  }
  return sum == n_trees && y < static_cast<unsigned>(C) ? static_cast<int>(y) * C + arg : -1;
}

// CW == 0: the binary form (one word per row).
template <int NW, int CW>
__global__ __launch_bounds__(NW * 64) void forest_eval_blocked_kernel(EvalArgs A, const float* __restrict__ xb,
                                                                      const unsigned char* __restrict__ prep,
                                                                      int fu_max, int64_t n_tiles) {
  constexpr int NT = NW * 64;
  constexpr int EW = CW ? CW : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n_inner = (1 << A.depth) - 1, n_leaf = 1 << A.depth;
  const BlockedPrepLayout L = blocked_prep_layout(A.n_trees, A.depth, fu_max);
  float* xs = reinterpret_cast<float*>(smem);
  unsigned char* fs = smem + static_cast<size_t>(fu_max) * kBlk * 4;  // the prepared payload
  const uint8_t* ls = fs + L.nodes;
  const uint16_t* used = reinterpret_cast<const uint16_t*>(fs + L.nodes + L.leaves);
  unsigned* s_hist = reinterpret_cast<unsigned*>(fs + L.payload);  // (16-B aligned)
  unsigned* ex = s_hist + round_up(A.n_cells, 4);                   // (16-B aligned)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < A.n_cells; i += NT) s_hist[i] = 0u;
  {
    // the prepared payload -> LDS, 16 B per thread, kPrepBatch loads in flight
    // (forest.hip's loop)
    constexpr int kPrepBatch = 4;
    const int n16 = static_cast<int>(L.payload >> 4);
    const uint4* src = reinterpret_cast<const uint4*>(prep + 16);
    uint4* dst = reinterpret_cast<uint4*>(fs);
    for (int e0 = tid; e0 < n16; e0 += kPrepBatch * NT) {
      uint4 q[kPrepBatch];
#pragma unroll
      for (int j = 0; j < kPrepBatch; ++j) q[j] = e0 + j * NT < n16 ? src[e0 + j * NT] : uint4{};
#pragma unroll
      for (int j = 0; j < kPrepBatch; ++j)
        if (e0 + j * NT < n16) dst[e0 + j * NT] = q[j];
    }
  }
  int fu = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(prep));
  fu = fu < fu_max ? fu : fu_max;  // (the buffer's own bound: the tile holds fu_max runs)
  __syncthreads();
  const int n_ins = blocked_dma_count(fu);  // DMA instructions per tile (4 runs each)
  typedef __attribute__((address_space(3))) float lds_float;
  typedef __attribute__((address_space(3))) const unsigned char lds_u8;
  const ByteWalk W{static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_u8*)fs)),
                   static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_u8*)ls)),
                   static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_float*)(xs + lane))),
                   NW, n_inner, n_leaf, A.depth};
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // block-uniform
    const int64_t row = tile * kBlk + lane;
    const bool live = row < A.n;
    // the row leader's label and flags are loaded with the tile
    unsigned y_pre = 255u;
    uint8_t fl_pre = DAL_ROW_CANDIDATE;
    if (wave == 0 && live) {
      y_pre = A.labels[row];
      if (A.flags) fl_pre = A.flags[row];
    }
    const char* src = reinterpret_cast<const char*>(xb + tile * A.d * kBlk);
    // (every wave stages, as in the binary score kernel: wave 0's epilogue is a
    // few LDS operations, not the score kernels' row stores)
    for (int i = wave; i < n_ins; i += NW) stage_blocked_runs(xs, src, used, fu, i, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned w[EW];
#pragma unroll
    for (int j = 0; j < EW; ++j) w[j] = 0u;
    if (live) {
      // groups of ILP trees, then the wave's last trees as ONE group of their count
      [[maybe_unused]] unsigned any = 0u;
      auto vote = [&](unsigned c) {
        if constexpr (CW == 0) {
          w[0] += c;
          any |= c;
        } else {
          add_vote<EW>(w, c);
        }
      };
      for (int t = wave; t < A.n_trees; t += kEvIlp * NW) {  // (wave-uniform)
        const int rem = (A.n_trees - t + NW - 1) / NW;
        if (rem >= kEvIlp) walk_group<kEvIlp>(W, t, vote);
        else walk_tail<kEvIlp - 1>(W, t, rem, vote);
      }
      if constexpr (CW == 0) w[0] = binary_word(w[0], any);
    }
    // a row's NW partial words, one set per wave, added through LDS (a field's
    // total <= T: no carry between fields)
    // (the binary form's words fit 16 bits: half the region, see eval_plan)
    [[maybe_unused]] unsigned short* ex16 = reinterpret_cast<unsigned short*>(ex);
    if (wave != 0) {
      if constexpr (CW == 0) {
        ex16[(wave - 1) * kBlk + lane] = static_cast<unsigned short>(w[0]);
      } else {
#pragma unroll
        for (int j = 0; j < EW; ++j) ex[((wave - 1) * EW + j) * kBlk + lane] = w[j];
      }
    }
    __syncthreads();  // ... and every walk of this tile is over: the next tile may be staged
    if (wave == 0) {
#pragma unroll
      for (int q = 0; q < NW - 1; ++q) {
        if constexpr (CW == 0) {
          w[0] += ex16[q * kBlk + lane];
        } else {
#pragma unroll
          for (int j = 0; j < EW; ++j) w[j] += ex[(q * EW + j) * kBlk + lane];
        }
      }
      int cell = -1;
      if (live && (fl_pre & DAL_ROW_CANDIDATE)) {
        if constexpr (CW == 0) cell = binary_cell(w[0], y_pre);
        else cell = multiclass_cell<EW>(w, A.n_classes, A.n_trees, y_pre);
      }
      table_add(s_hist, cell, lane);
    }
  }
  __syncthreads();
  for (int i = tid; i < A.n_cells; i += NT)
    if (s_hist[i]) atomicAdd(&A.hist[i], static_cast<unsigned long long>(s_hist[i]));
}

// The row-major form: one thread per row over x, the forest from global memory
// (a few KiB, resident in the caches).  A node feature outside [0, d) is
// clamped, as the blocked kernels do.
template <int CW>
__global__ __launch_bounds__(kEvRowThreads) void forest_eval_rows_kernel(EvalArgs A, const float* __restrict__ x,
                                                                         int64_t ldx,
                                                                         const int2* __restrict__ inner,
                                                                         const uint8_t* __restrict__ leaf) {
  constexpr int EW = CW ? CW : 1;
  extern __shared__ unsigned s_hist[];
  for (int i = threadIdx.x; i < A.n_cells; i += kEvRowThreads) s_hist[i] = 0u;
  __syncthreads();
  const int n_inner = (1 << A.depth) - 1, n_leaf = 1 << A.depth;
  const int lane = threadIdx.x & 63;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kEvRowThreads;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * kEvRowThreads; base < A.n; base += stride) {  // block-uniform
    const int64_t row = base + threadIdx.x;
    int cell = -1;
    if (row < A.n && (!A.flags || (A.flags[row] & DAL_ROW_CANDIDATE))) {
      const unsigned y = A.labels[row];
      const float* xr = x + row * ldx;
      unsigned w[EW];
#pragma unroll
      for (int j = 0; j < EW; ++j) w[j] = 0u;
      [[maybe_unused]] unsigned any = 0u;
      for (int t = 0; t < A.n_trees; ++t) {
        const int2* nodes = inner + static_cast<int64_t>(t) * n_inner;
        int h = 0;
        for (int lvl = 0; lvl < A.depth; ++lvl) {
          const int2 nd = nodes[h];
          const int f = nd.x < 0 ? 0 : nd.x >= A.d ? A.d - 1 : nd.x;
          h = 2 * h + (xr[f] <= __int_as_float(nd.y) ? 1 : 2);
        }
        const unsigned c = leaf[static_cast<int64_t>(t) * n_leaf + (h - n_inner)];
        if constexpr (CW == 0) {
          w[0] += c;
          any |= c;
        } else {
          add_vote<EW>(w, c);
        }
      }
      if constexpr (CW == 0) cell = binary_cell(binary_word(w[0], any), y);
      else cell = multiclass_cell<EW>(w, A.n_classes, A.n_trees, y);
    }
    table_add(s_hist, cell, lane);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < A.n_cells; i += kEvRowThreads)
    if (s_hist[i]) atomicAdd(&A.hist[i], static_cast<unsigned long long>(s_hist[i]));
}

// The applicability rule and the launch shape of the blocked kernel: the score
// kernels' rule for this forest (their prepared buffer is this kernel's), and
// the block's LDS with the table and the exchange region within the 96 KiB the
// score rules allow themselves; 8 waves when four-wave blocks fit at most two
// per CU (their threshold).
struct EvalPlan {
  int fu_max = 0;  // 0: the blocked kernel does not apply
  int nw = 0;
  size_t smem = 0;
};
EvalPlan eval_plan(int64_t d, int32_t n_trees, int32_t depth, int32_t n_classes) {
  EvalPlan P;
  const int cells = dal_forest_evaluate_cells(n_trees, n_classes);
  if (!cells || d < 1 || depth < 1 || depth > DAL_MAX_TREE_DEPTH) return P;
  const int rows = n_classes > 2 ? dal_forest_multiclass_blocked_rows(d, n_trees, depth, n_classes)
                                 : dal_forest_blocked_rows(d, n_trees, depth);
  if (!rows) return P;
  const int64_t nodes = static_cast<int64_t>(n_trees) * ((int64_t{1} << depth) - 1);
  const int64_t fu = nodes < d ? nodes : d;
  const BlockedPrepLayout L = blocked_prep_layout(n_trees, depth, fu);
  const size_t base = static_cast<size_t>(fu) * kBlk * 4 + static_cast<size_t>(L.payload) +
                      static_cast<size_t>(round_up(cells, 4)) * 4;
  // one wave's partial words: CW 32-bit words per row, 16 bits in the binary
  // form -- with 32 there, 256 tested features under 100 trees came to 82,256
  // bytes, 336 past half a CU's LDS: one block per CU where the score kernel
  // has two (2M x 256, T = 100: 533 us against its 408)
  const size_t row_bytes = n_classes > 2 ? static_cast<size_t>(mc_words(n_classes)) * kBlk * 4 : kBlk * 2;
  const bool wide = base + (kEvWaves - 1) * row_bytes > (160u << 10) / 3;
  const int nw = wide ? kEvWavesWide : kEvWaves;
  const size_t smem = base + (nw - 1) * row_bytes;
  if (smem > 96 * 1024) return P;
  P.fu_max = static_cast<int>(fu);
  P.nw = nw;
  P.smem = smem;
  return P;
}

template <int CW>
int eval_launch_blocked(const EvalArgs& A, const float* xb, const void* fprep, const EvalPlan& P, hipStream_t st) {
  const int64_t tiles = ceil_div(A.n, kBlk);
  const bool wide = P.nw == kEvWavesWide;
  const auto kern = wide ? &forest_eval_blocked_kernel<kEvWavesWide, CW> : &forest_eval_blocked_kernel<kEvWaves, CW>;
  // a persistent grid of the blocks resident at once: every block stages the
  // forest once and flushes its table once
  const int64_t grid = persistent_grid(reinterpret_cast<const void*>(kern), P.nw * 64, P.smem, kEvPerCu, tiles);
  if (grid < 0) return static_cast<int>(grid);
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(P.nw * 64), P.smem, st, A, xb,
                     static_cast<const unsigned char*>(fprep), P.fu_max, tiles);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

template <int CW>
int eval_launch_rows(const EvalArgs& A, const float* x, int64_t ldx, const int32_t* inner, const uint8_t* leaf,
                     hipStream_t st) {
  int64_t blocks = ceil_div(A.n, kEvRowThreads);
  blocks = blocks > 4096 ? 4096 : blocks;
  hipLaunchKernelGGL(forest_eval_rows_kernel<CW>, dim3(static_cast<unsigned>(blocks)), dim3(kEvRowThreads),
                     static_cast<size_t>(A.n_cells) * sizeof(unsigned), st, A, x, ldx,
                     reinterpret_cast<const int2*>(inner), leaf);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" int dal_forest_evaluate_cells(int32_t n_trees, int32_t n_classes) {
  if (n_classes == 2) return n_trees >= 1 && n_trees <= DAL_LAL_MAX_TREES ? (n_trees + 1) * 2 : 0;
  if (n_classes < 3 || n_classes > DAL_MC_MAX_CLASSES || n_trees < 1 || n_trees > DAL_MC_MAX_TREES) return 0;
  return n_classes * n_classes;
}

extern "C" int dal_forest_evaluate_blocked_rows(int64_t d, int32_t n_trees, int32_t depth, int32_t n_classes) {
  return eval_plan(d, n_trees, depth, n_classes).fu_max ? kBlk : 0;
}

extern "C" int dal_forest_evaluate(const float* x, const float* xb, const void* fprep, int64_t n, int64_t d,
                                   int64_t ldx, const int32_t* inner, const uint8_t* leaf, int32_t n_trees,
                                   int32_t depth, int32_t n_classes, const uint8_t* labels,
                                   const uint8_t* row_flags, int64_t* hist, dal_stream_t stream) {
  if (!x || !inner || !leaf || !labels || !hist) return DAL_ERR_ARG;
  // (the 32-bit LDS counters of a block cannot wrap below 2^32 rows)
  if (n < 0 || n > int64_t{0xFFFFFFFF} || d < 1 || ldx < d || d > (int64_t{1} << 30)) return DAL_ERR_SHAPE;
  if (depth < 1 || depth > DAL_MAX_TREE_DEPTH) return DAL_ERR_UNSUPPORTED;
  const int cells = dal_forest_evaluate_cells(n_trees, n_classes);
  if (!cells) return DAL_ERR_UNSUPPORTED;
  const EvalPlan P = xb ? eval_plan(d, n_trees, depth, n_classes) : EvalPlan{};
  if (xb && reinterpret_cast<uintptr_t>(xb) % 16 != 0) return DAL_ERR_ARG;
  if (P.fu_max && (!fprep || reinterpret_cast<uintptr_t>(fprep) % 16 != 0)) return DAL_ERR_ARG;
  if (n == 0) return DAL_OK;
  const EvalArgs A{n, static_cast<int>(d), n_trees, depth, n_classes, cells, labels, row_flags,
                   reinterpret_cast<unsigned long long*>(hist)};
  const hipStream_t st = as_stream(stream);
  if (n_classes == 2)
    return P.fu_max ? eval_launch_blocked<0>(A, xb, fprep, P, st) : eval_launch_rows<0>(A, x, ldx, inner, leaf, st);
  return dispatch_cw(n_classes, [&](auto cw) {
    constexpr int CW = decltype(cw)::value;
    return P.fu_max ? eval_launch_blocked<CW>(A, xb, fprep, P, st) : eval_launch_rows<CW>(A, x, ldx, inner, leaf, st);
  });
}
