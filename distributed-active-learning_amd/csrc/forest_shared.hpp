// What the forest score kernels share (forest.hip, forest_multi.hip,
// forest_multi_blocked.hip): the prepared forest's layout, the density power
// and its error bound, the packed class counters and the C-class row epilogue,
// the byte-addressed tree walk, one DMA instruction of the blocked tile's
// staging, the row-major tiling rule, and the launchers' grid sizing, argument
// checks and class-width dispatch.  One definition each; every kernel
// instantiates what it uses.  The condition on this header: the binary kernels
// (forest.hip) and the blocked multiclass kernels compile from it to the
// instructions they had with private copies, and the row-major multiclass
// kernels to the same registers, scratch and LDS -- scripts/isa_diff.py
// against the commit before compares every kernel (profiles/forest_shared/).
#pragma once

#include <type_traits>

#include "common.hpp"

namespace dal {
namespace {

// Rows per tile of the pool's blocked feature-major copy (dal_pool_blocked).
constexpr int kBlk = 64;

// The prepared forest (dal_forest_prepare): a 16-B header {fu, bad, nn,
// fu_max} then the payload [nodes int2 nn (feature -> byte offset slot * kBlk
// * 4 of its run in the LDS tile) | leaves u8 round4(T * 2^depth) | feature
// list u16 round2(fu_max)], zero-padded to 16 B: the blocked kernels' LDS
// layout from their forest region on.
struct BlockedPrepLayout {
  int64_t nodes, leaves, used, payload, total;
};
__host__ __device__ inline BlockedPrepLayout blocked_prep_layout(int64_t n_trees, int32_t depth, int64_t fu_max) {
  BlockedPrepLayout L;
  L.nodes = n_trees * ((int64_t{1} << depth) - 1) * 8;
  L.leaves = round_up(n_trees << depth, 4);
  L.used = round_up(fu_max, 2) * 2;
  L.payload = round_up(L.nodes + L.leaves + L.used, 16);
  L.total = 16 + L.payload;
  return L;
}

// density^beta for beta != 1, called out of line: inlined, pow's registers
// counted against every score kernel's occupancy although beta == 1 in the
// common case, where no call is made (the binary blocked kernel 101 -> 74
// VGPRs, 4 -> 6 waves per SIMD).  The binary kernels test beta at run time;
// the multiclass launchers pick the kernel by beta (POW): their beta == 1
// kernels hold no call at all -- a call that is never taken still cost them
// 1 % (config 4, T = 10) to 3 % (T = 100) and 8 bytes of scratch per lane.
__device__ __attribute__((noinline)) double density_pow_general(double d, double beta) { return pow(d, beta); }
template <bool POW>
__device__ __forceinline__ double density_pow_if(double d, double beta) {
  if constexpr (POW) return density_pow_general(d, beta);
  return d;
}

// |d^beta - d'^beta| bound for |d - d'| <= derr.
__device__ __attribute__((noinline)) double density_pow_err_general(double d, double derr, double beta) {
  const double p = pow(fabs(d), beta);
  const double hi = pow(fabs(d) + derr, beta);
  const double lo = pow(fmax(fabs(d) - derr, 0.0), beta);
  return fmax(fabs(hi - p), fabs(p - lo)) * (1.0 + 1e-12) + fabs(p) * 1e-14;
}
template <bool POW>
__device__ __forceinline__ double density_pow_err_if(double d, double derr, double beta) {
  if constexpr (POW) return density_pow_err_general(d, derr, beta);
  return derr;
}

// ------------------------------------------------- packed class counters --
// A row's C class counts as 8-bit fields, four per 32-bit word, in CW words
// (every word index a compile-time constant, so the words stay in registers).
// One vote for class c: 1 << 8 (c & 3) added to word c >> 2.  The loop is
// unrolled over the CW words (a runtime-indexed register array would live in
// scratch); a class >= 4 CW matches no word and is dropped.  (A bit extract
// from a one-hot word mask and a shift-add per word, 2 VALU instead of 3,
// measured the same: config 3 56.3 -> 56.5 us.)
template <int CW>
__device__ __forceinline__ void add_vote(unsigned (&w)[CW], unsigned c) {
  const unsigned inc = 1u << (8u * (c & 3u));
  const unsigned word = c >> 2;
#pragma unroll
  for (int j = 0; j < CW; ++j) w[j] += word == static_cast<unsigned>(j) ? inc : 0u;
}

template <int CW>
__device__ __forceinline__ int vote_field(const unsigned (&w)[CW], int c) {  // c: a compile-time constant at every call
  return static_cast<int>((w[c >> 2] >> (8 * (c & 3))) & 255u);
}

// The multiclass row leader's epilogue: w holds the row's C counts.  Args: a
// kernel's McArgs, or with DW its McDwArgs (fl_pre: the row's flags; dens_pre:
// its density word, both loaded with the tile).  Hands back the row's interval
// keys (DW; DAL_KEY_NONE for a non-candidate) for the step kernels' group fold.
struct RowKeys {
  unsigned long long lo = DAL_KEY_NONE, hi = DAL_KEY_NONE;
};
template <int CW, bool DW, bool POW, class Args>
__device__ __forceinline__ RowKeys row_epilogue(const Args& A, const unsigned (&w)[CW], int64_t row, uint8_t fl_pre,
                                                long long dens_pre, const double* lut_s) {
  const int C = A.n_classes;
  // largest and second-largest count, the lowest class holding the largest
  int m1 = -1, m2 = -1, arg = 0;
#pragma unroll
  for (int c = 0; c < 4 * CW; ++c) {
    if (c < C) {
      const int nc = vote_field<CW>(w, c);
      if (nc > m1) {
        m2 = m1;
        m1 = nc;
        arg = c;
      } else if (nc > m2) {
        m2 = nc;
      }
    }
  }
  double s;
  if (DW || A.kind == DAL_MC_ENTROPY) {
    s = 0.0;
#pragma unroll
    for (int c = 0; c < 4 * CW; ++c)
      if (c < C) s = __dadd_rn(s, lut_s[vote_field<CW>(w, c)]);  // class order, one rounding per add
  } else {
    s = lut_s[A.kind == DAL_MC_MARGIN ? m1 - m2 : m1];
  }
  if (A.counts) {
    // the packed words are the row's count bytes in memory order (little
    // endian): whole words or halves where C and the buffer's alignment allow
    uint8_t* cr = A.counts + row * C;
    if (A.cstore == 4) {
#pragma unroll
      for (int j = 0; j < CW; ++j)
        if (4 * j < C) reinterpret_cast<uint32_t*>(cr)[j] = w[j];
    } else if (A.cstore == 2) {
#pragma unroll
      for (int hw = 0; hw < 2 * CW; ++hw)
        if (2 * hw < C) reinterpret_cast<uint16_t*>(cr)[hw] = static_cast<uint16_t>(w[hw >> 1] >> (16 * (hw & 1)));
    } else {
#pragma unroll
      for (int c = 0; c < 4 * CW; ++c)
        if (c < C) cr[c] = static_cast<uint8_t>(vote_field<CW>(w, c));
    }
  }
  if (A.pred) A.pred[row] = static_cast<uint8_t>(arg);
  if constexpr (DW) {
    // the binary kernel's density epilogue (forest.hip) on the class entropy
    // e (never NaN, >= +0.0): s = e d^beta, descending, and for the GEMM
    // density the interval s -+ e err(d^beta) as two keys
    const double e = s;
    double d = A.dkind == DAL_DENSITY_FIXED ? from_fixed(dens_pre) : __builtin_bit_cast(double, dens_pre);
    if (fl_pre & DAL_ROW_EXCLUDED) d = __builtin_nan("");
    s = e * density_pow_if<POW>(d, A.beta);
    double err = 0.0;
    if (A.dkind == DAL_DENSITY_FIXED && e != 0.0 && d == d) {
      err = e * density_pow_err_if<POW>(d, A.derr, A.beta);
      // keep the interval ends distinct from s after rounding
      err = fmax(err, fabs(s) * 4.5e-16);
    }
    unsigned long long klo = DAL_KEY_NONE, khi = DAL_KEY_NONE;
    if (fl_pre & DAL_ROW_CANDIDATE) {
      klo = score_key(pessimistic(s, err, DAL_DESCENDING), DAL_DESCENDING);
      khi = score_key(optimistic(s, err, DAL_DESCENDING), DAL_DESCENDING);
    }
    A.entropy[row] = e;
    A.row_index[row] = static_cast<int32_t>(row);  // (n <= INT32_MAX, checked by the entry)
    A.scores[row] = s;
    A.keys[row] = klo;
    if (A.keys_hi) A.keys_hi[row] = khi;
    return RowKeys{klo, khi};
  } else {
    A.scores[row] = s;
    A.keys[row] = (fl_pre & DAL_ROW_CANDIDATE) ? score_key(s, A.order) : DAL_KEY_NONE;
    return RowKeys{};
  }
}

// The row leader's flags in a step kernel of the multiclass forms
// (ForestStepHooks, forest.hip's row_flag): row_flags[row], or for a plan the
// pool's base flags with DAL_ROW_CANDIDATE from this step's mark stamp --
// written to row_flags for the step's later kernels when write_flags is set.
__device__ __forceinline__ uint8_t step_row_flag(const ForestStepHooks& H, const uint8_t* flags, int64_t row) {
  if (!H.base_flags) return flags ? flags[row] : static_cast<uint8_t>(DAL_ROW_CANDIDATE);
  const bool cand = H.stamp[row] == static_cast<uint8_t>(*H.step_id);
  const uint8_t fl = static_cast<uint8_t>(H.base_flags[row] | (cand ? DAL_ROW_CANDIDATE : 0));
  if (H.write_flags && flags) const_cast<uint8_t*>(flags)[row] = fl;
  return fl;
}

// ------------------------------------------------- byte-addressed walks --
// Walks of M trees (t, t + tpr, ...) at once for one row over the prepared
// forest in LDS: node h of tree t sits at LDS byte tb + 8 h, so its child
// 2h + 1 (x <= thr) or 2h + 2 sits at 2a + (8 - tb) or 2a + (16 - tb) -- a
// select and a shift-add per level; the leaf byte at (a >> 3) + lbase +
// t * n_leaf - n_inner - tb / 8.  visit(leaf byte) once per tree: the binary
// kernel sums the bytes, the multiclass kernel votes each as a class id.  The
// visitor (a lambda holding a reference to the caller's accumulator) is taken
// by value: by forwarding reference both blocked kernels compiled to other
// code (the multiclass DW ones to other register counts).
struct ByteWalk {
  unsigned fbase, lbase, xb;  // LDS byte addresses: nodes, leaves, this row's x
  int tpr, n_inner, n_leaf, depth;
};
template <int M, class Visit>
__device__ __forceinline__ void walk_group(const ByteWalk& W, int t, Visit visit) {
  typedef __attribute__((address_space(3))) const float lds_float;
  typedef __attribute__((address_space(3))) const uint8_t lds_u8;
  typedef __attribute__((address_space(3))) const unsigned long long lds_u64;
  unsigned a[M], kl[M], kr[M], lo[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int tj = t + j * W.tpr;
    const unsigned tb = W.fbase + static_cast<unsigned>(8 * tj * W.n_inner);
    a[j] = tb;
    kl[j] = 8u - tb;
    kr[j] = 16u - tb;
    lo[j] = W.lbase + static_cast<unsigned>(tj * W.n_leaf - W.n_inner) - (tb >> 3);
    // opaque to the optimiser and held in vector registers, so the step stays
    // select + shift-add instead of shift, subtract, select, add
    asm volatile("" : "+v"(kl[j]), "+v"(kr[j]));
  }
  for (int lvl = 0; lvl < W.depth; ++lvl) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const unsigned long long nd = *(lds_u64*)static_cast<uintptr_t>(a[j]);  // {feature run offset, thr}
      const float xv = *(lds_float*)static_cast<uintptr_t>(W.xb + static_cast<unsigned>(nd));
      a[j] = 2u * a[j] + (xv <= __uint_as_float(static_cast<unsigned>(nd >> 32)) ? kl[j] : kr[j]);
    }
  }
  unsigned c[M];
#pragma unroll
  for (int j = 0; j < M; ++j) c[j] = *(lds_u8*)static_cast<uintptr_t>((a[j] >> 3) + lo[j]);
#pragma unroll
  for (int j = 0; j < M; ++j) visit(c[j]);
}
// the last rem (<= M) trees of a wave as one group (rem wave-uniform)
template <int M, class Visit>
__device__ __forceinline__ void walk_tail(const ByteWalk& W, int t, int rem, Visit visit) {
  if constexpr (M > 0) {
    if (rem == M) walk_group<M>(W, t, visit);
    else walk_tail<M - 1>(W, t, rem, visit);
  }
}

// ------------------------------------------------------------- staging --
// A 64-row tile of the blocked copy -> LDS by LDS-DMA: only the 256-B runs of
// the forest's fu listed features (used[], in LDS), four runs per
// global_load_lds_dwordx4 (lane l loads 16 B of run 4i + l / 16), so
// blocked_dma_count(fu) instructions per tile.  stage_blocked_runs issues
// instruction i (wave-uniform) from tile_src, the tile's first run; which wave
// issues which i is the kernel's choice, and so the loop over i is the
// kernel's (as are the loops of the prepared payload's copy and of the
// row-major staging: inside a helper they compile to other instructions than
// the binary kernels had, by order and register names only, and those kernels
// are held to the instructions they had).
__device__ __forceinline__ int blocked_dma_count(int fu) { return (fu + 3) >> 2; }
__device__ __forceinline__ void stage_blocked_runs(float* xs, const char* tile_src, const uint16_t* used, int fu, int i,
                                                   int lane) {
  typedef __attribute__((address_space(3))) float lds_float;
  const int sl = 4 * i + (lane >> 4);
  const unsigned dst = __builtin_amdgcn_readfirstlane(
      static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_float*)(xs + 4 * i * kBlk))));
  if (sl < fu) {
    const unsigned voff = static_cast<unsigned>(used[sl]) * (kBlk * 4u) + static_cast<unsigned>(lane & 15) * 16u;
    lds_dma_x4(voff, dst, tile_src);
  }
}

// ---------------------------------------------------------- host side --
#ifndef DAL_FOREST_TPR
#define DAL_FOREST_TPR 2
#endif

// The row-major kernels' tile (blocks of `threads` threads).
struct ForestTiling {
  int R;       // rows per block
  bool x_lds;  // pool rows staged in LDS
  bool dma;    // ... by LDS-DMA (wide rows)
};
inline ForestTiling forest_tiling(const float* x, int64_t d, int64_t ldx, int32_t n_trees, int threads) {
  // rows per block: stage up to ~16 KiB of pool rows in LDS.  Small tiles keep
  // more blocks (and their loads) resident per CU: at 2M x 256 a 16 KiB tile
  // runs 0.52 ms vs 0.60 (32 KiB) / 0.85 (96 KiB) / 0.75 (8 KiB); neutral at
  // 100k x 64 and 284,807 x 30
  ForestTiling T{256, true, false};
  // LDS-DMA staging for wide rows (d % 4 == 0, ldx % 4 == 0, 16-B-aligned
  // pool; narrow rows leave most lanes of each DMA instruction idle: 2M x 32 x
  // 100: 264 -> 290 us, 100k x 64: 18.4 -> 19.8) holds no registers: 32 KiB
  // tiles there (2M x 256: 441 -> 411 us; 64 KiB 1248)
  T.dma = d >= 128 && d % 4 == 0 && ldx % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
  const int64_t tile_cap = T.dma ? 33280 : 16640 * (threads / 256);
  while (T.R > 16 && static_cast<int64_t>(T.R) * (d + 1) * 4 > tile_cap) T.R >>= 1;
  // wide rows: 16 rows may exceed the preferred tile; LDS staging up to 64 KiB
  if (static_cast<int64_t>(T.R) * (d + 1) * 4 > 65536) {
    T.x_lds = false;
    T.dma = false;
    T.R = 256;
  }
  // many trees (config 3: T = 100): spread a row's trees over more lanes --
  // the traversal's dependent LDS round trips, not HBM, bound that case
  const int tpr_min = n_trees >= 64 ? DAL_FOREST_TPR : 1;  // config 3: 60.7 -> 51.8 us (4: 53.5, 8: 60.9)
  if (T.x_lds) {
    while (T.R > 1 && threads / T.R < tpr_min) T.R >>= 1;
  }
  return T;
}

// A persistent grid for kernel fn (blocks of `threads`, smem bytes of dynamic
// LDS, which fn is allowed here): exactly the blocks resident at once
// (registers, LDS, waves: the occupancy query -- a grid past it would start
// its extra blocks only when others END), per_cu_cap per CU at most (0: no
// cap), and no more than `tiles`.  Returns the grid, or DAL_ERR_HIP.
inline int64_t persistent_grid(const void* fn, int threads, size_t smem, int per_cu_cap, int64_t tiles) {
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1 ||
      hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem)) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, smem) != hipSuccess)
    return DAL_ERR_HIP;
  if (per_cu_cap > 0 && per_cu > per_cu_cap) per_cu = per_cu_cap;
  if (per_cu < 1) per_cu = 1;
  const int64_t resident = static_cast<int64_t>(cus) * per_cu;
  return tiles < resident ? tiles : resident;
}

// What every multiclass entry checks, in the order they all report it:
// DAL_ERR_ARG (args_ok: the entry's own null-operand and enum tests) before
// DAL_ERR_SHAPE before DAL_ERR_UNSUPPORTED.  index32: the entry writes int32
// row indices (the density-weighted forms).
inline int mc_validate(bool args_ok, int64_t n, int64_t d, int64_t ldx, int32_t n_trees, int32_t depth,
                       int32_t n_classes, bool index32) {
  if (!args_ok) return DAL_ERR_ARG;
  if (n < 0 || d < 1 || ldx < d || d > (int64_t{1} << 30)) return DAL_ERR_SHAPE;
  if (index32 && n > INT32_MAX) return DAL_ERR_SHAPE;  // row_index is int32 (dal_dw_select's vote type)
  if (depth < 1 || depth > DAL_MAX_TREE_DEPTH) return DAL_ERR_UNSUPPORTED;
  if (n_classes < 2 || n_classes > DAL_MC_MAX_CLASSES) return DAL_ERR_UNSUPPORTED;
  if (n_trees < 1 || n_trees > DAL_MC_MAX_TREES) return DAL_ERR_UNSUPPORTED;
  return DAL_OK;
}

// The uncertainty forms' enums (part of their args_ok).
inline bool mc_uncertainty_enums_ok(int order, int score_kind) {
  return (order == DAL_ASCENDING || order == DAL_DESCENDING) &&
         (score_kind == DAL_MC_LEAST_CONFIDENCE || score_kind == DAL_MC_MARGIN || score_kind == DAL_MC_ENTROPY);
}

// Bytes per store of a row's counts: 4, 2 or 1, by C and the buffer's alignment.
inline int mc_cstore(const uint8_t* counts, int32_t n_classes) {
  const uintptr_t ca = reinterpret_cast<uintptr_t>(counts);
  return (n_classes % 4 == 0 && ca % 4 == 0) ? 4 : (n_classes % 2 == 0 && ca % 2 == 0) ? 2 : 1;
}

// Words of packed counters for C classes: CW = 1, 2, 4, 8 for C <= 4, 8, 16, 32.
constexpr int mc_words(int32_t n_classes) { return n_classes <= 4 ? 1 : n_classes <= 8 ? 2 : n_classes <= 16 ? 4 : 8; }
// f(std::integral_constant<int, CW>{}) for the CW of n_classes.
template <class F>
inline int dispatch_cw(int32_t n_classes, F&& f) {
  switch (mc_words(n_classes)) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

}  // namespace
}  // namespace dal
