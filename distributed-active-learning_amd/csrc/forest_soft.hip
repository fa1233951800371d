// Soft-vote random forests: the averaged leaf class distribution of every
// pool row (scikit-learn's RandomForestClassifier.predict_proba, modAL's
// uncertainty measures, spark.ml's probabilityCol) fused with the uncertainty
// score, exact.
//
// A leaf holds its class distribution as C fixed-point words q[c] =
// rint(p[c] 2^31) (uint32, <= 2^31).  A row's class sums S_c = sum_t
// q[leaf_t(row)][c] are exact integers below 2^39, so any launch shape, lane
// mapping, row order or shard count gives the same bytes; the scores are one
// IEEE division of two exactly representable integers (least confidence,
// margin) or the class-ordered entropy of the C quotients ("K2 soft
// votes").
//
// MI355X design: the row-major multiclass kernel's (forest_multi.hip) -- an HBM
// stream; a block stages R pool rows in LDS (LDS-DMA for wide aligned rows on
// a persistent grid, 16-B or scalar loads for narrow rows, rows from global
// memory when 16 of them exceed 64 KiB), the forest is LDS-resident when its
// nodes, leaf ids and padded leaf table fit 64 KiB, and tpr = 256 / R threads
// share a row, each walking every tpr-th tree with 4 traversals in flight.
// What differs is the accumulator: W 64-bit integer sums per lane (W = 2, 4,
// 8, 16, 32 for C <= 2, 4, 8, 16, 32; a template parameter, every index a
// compile-time constant, so the sums stay in registers), added across a row's
// lanes with integer __shfl_xor adds.  In LDS a leaf's words sit in a row of
// round2(C) words, zero padded and 8-B aligned, so a leaf is read in 8-byte
// pieces; from global memory the caller's [L, C] table is read word by word.
// The entropy's C divisions and logarithms are spread over the row's tpr lanes
// (on the row leader alone they idle the other lanes for most of the kernel's
// time at C = 10) and added in class order.
// The staging loops are this kernel's own copies of the forms of
// forest_multi_body.inc (the existing kernels are held to the instructions
// they have; forest_shared.hpp is included unchanged).
//
// The density-weighted form (DW; dal_forest_score_soft_dw, and under
// dal_dw_step_soft) is modAL's information density on predict_proba: the same
// walk, accumulators, staging and entropy (forest_soft_body.inc, one text for
// both kernels), and a row-leader epilogue that multiplies the class entropy
// by density^beta and writes the interval keys of the hard-vote density
// kernels, plus the row's entropy and its own index, so that dal_dw_select
// (lut = entropy, votes = index) re-ranks it unchanged.  The row leader's
// density word is loaded with its flags when the tile is staged; the
// epilogue's fp64 temporaries exist after the cross-lane sum only.  The DW =
// false kernels are the code they were without it.
//
// The BALD form (dal_forest_score_soft_bald) scores the trees' disagreement,
// H(pbar) - (1/T) sum_t H(p_t): a leaf's entropy is one more fixed-point word
// (leaf_h, rint(H_l 2^29)) and a row's sum of them one more exact 64-bit
// integer per lane, added across the row's lanes like the class sums.  In LDS
// the word sits at column C of the leaf's row of round2(C + 1) words (for odd
// C the padding word that was there already) and arrives in the 8-byte reads
// the row takes anyway; from global memory it comes from the caller's [L]
// array.  (For odd C the reads, the adds and the cross-lane sum are the class
// sums' own: the word lands in the spare accumulator s[C].)  The row leader
// forms entropy - hsum / (T 2^29), clamped at +0.0.
// Everything it adds is gated by `if constexpr (BALD)`: the other kernels are
// the code they were.
#include "forest_shared.hpp"

namespace dal {
namespace {

constexpr int kSoftThreads = 256;
constexpr int kSoftIlp = 4;                   // independent tree walks in flight per lane
constexpr int64_t kSoftForestLds = 65536;     // LDS budget of the resident forest
constexpr int64_t kSoftMaxLeaves = 1 << 26;   // n_leaves * 32 classes stays below 2^31

struct SoftArgs {
  const float* x;
  int64_t n;
  int d;
  int64_t ldx;
  const int2* inner;
  const int32_t* leaf_id;
  const uint32_t* leaf_q;
  int n_leaves;
  int n_trees;
  int depth;
  int n_classes;
  int kind;
  const uint8_t* flags;
  int order;
  unsigned long long* sums;
  uint8_t* pred;
  double* scores;
  uint64_t* keys;
};

// The density-weighted form (dal_forest_score_soft_dw): the class entropy
// times density^beta with interval keys, the density epilogue of the hard-vote
// kernels (forest_shared.hpp, row_epilogue<.., DW = true, POW>) on the
// soft-vote entropy.  Its arguments extend SoftArgs (kind = DAL_SOFT_ENTROPY,
// order = DAL_DESCENDING, keys = the pessimistic keys), so the uncertainty
// form's kernels take the struct they always took.
struct SoftDwArgs : SoftArgs {
  const void* density;  // int64 fixed point (DAL_DENSITY_FIXED) or fp64 bits (DAL_DENSITY_EXACT), one word per row
  int dkind;
  double derr;
  double beta;
  double* entropy;
  int32_t* row_index;
  uint64_t* keys_hi;      // nullable
  int32_t* status_reset;  // nullable; dal_dw_step_soft: zeroed by the grid's first thread
};

// The BALD form (dal_forest_score_soft_bald): the entropy (kind =
// DAL_SOFT_ENTROPY) minus the mean of the reached leaves' entropies.
struct SoftBaldArgs : SoftArgs {
  const uint32_t* leaf_h;    // [n_leaves] rint(H_l 2^DAL_SOFT_ENTROPY_SHIFT)
  unsigned long long* hsum;  // nullable
  double* entropy;           // nullable
};

// Words per leaf row of the LDS copy of the leaf table: C rounded up to even,
// so a row is 8-byte aligned and read in 8-byte pieces.
__host__ __device__ inline int soft_lds_stride(int n_classes) { return (n_classes + 1) & ~1; }
// ... BALD: of the C class words and the leaf's entropy word at column C.
template <bool BALD>
__host__ __device__ inline int soft_lds_row(int n_classes) {
  return soft_lds_stride(n_classes + (BALD ? 1 : 0));
}
// Word c of leaf l's LDS row: the class word, (BALD) the entropy word at
// column C, zero padding after them.
template <bool BALD, class Args>
__device__ __forceinline__ uint32_t soft_lds_word(const Args& A, int l, int c) {
  if constexpr (BALD) {
    if (c == A.n_classes) return A.leaf_h[l];
  }
  return c < A.n_classes ? A.leaf_q[l * A.n_classes + c] : 0u;
}
// The caller's [L] array of leaf entropy words (BALD; nothing otherwise).
template <bool BALD, class Args>
__device__ __forceinline__ const uint32_t* soft_leaf_h(const Args& A) {
  if constexpr (BALD) return A.leaf_h;
  else return nullptr;
}

// s[c] += q[c], c < C, for the leaf whose words start at q: the padded LDS row
// in 8-byte pieces (Q_LDS; ds_read_b64 moves the bytes per LDS cycle of the
// wider reads, and rows of round2(C) words waste at most one word where 16-byte
// rows would waste up to three), or the caller's row word by word.
template <int W, bool Q_LDS>
__device__ __forceinline__ void add_leaf(unsigned long long (&s)[W], const uint32_t* q, int C) {
  if constexpr (Q_LDS) {
#pragma unroll
    for (int j = 0; j < W / 2; ++j) {
      if (2 * j < C) {  // (block-uniform; the padding word is zero)
        const uint2 v = reinterpret_cast<const uint2*>(q)[j];
        s[2 * j + 0] += v.x;
        s[2 * j + 1] += v.y;
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < W; ++c)
      if (c < C) s[c] += q[c];
  }
}

// BALD: add_leaf, and the leaf's entropy word.  Q_LDS: q is the leaf's row of
// round2(C + 1) words, the entropy word at column C.  Odd C (< W): the word is
// the second half of the last class piece, where add_leaf's row has its zero
// padding, and add_leaf's own 8-byte reads add it into s[C], the accumulator
// no class uses -- no read and no add beyond the entropy kernel's; the caller
// takes the row's sum from s[C] (soft_spare_sum).  Even C: the first word of
// one more piece, added into hs.  Otherwise (the caller's tables) the word is
// leaf_h[l], added into hs.
template <int W, bool Q_LDS>
__device__ __forceinline__ void add_leaf_bald(unsigned long long (&s)[W], unsigned long long& hs, const uint32_t* q,
                                              int C, const uint32_t* leaf_h, unsigned l) {
  add_leaf<W, Q_LDS>(s, q, C);
  if constexpr (Q_LDS) {
    if (!(C & 1)) hs += q[C];  // (block-uniform)
  } else {
    hs += leaf_h[l];
  }
}

// s[C] for odd C, read through a select over the W registers (compile-time
// indices): the sum of the entropy words add_leaf_bald left there.
template <int W>
__device__ __forceinline__ unsigned long long soft_spare_sum(const unsigned long long (&s)[W], int C) {
  unsigned long long v = 0ull;
#pragma unroll
  for (int j = 1; j < W; j += 2) v = j == C ? s[j] : v;
  return v;
}

// The class-ordered entropy of a row whose tpr lanes (consecutive, sub = the
// lane's place among them) all hold the row's sums s: lane sub forms the terms
// of classes sub, sub + tpr, ... (the division and the log2, the costly part,
// on every lane instead of on the row leader alone), and every lane adds the
// terms in class order, read from their lanes.  Called in block-uniform
// control flow; the same bits for every tpr.  The class picked at run time is
// read through a select over the W registers (compile-time indices).
template <int W>
__device__ __forceinline__ double soft_entropy(const unsigned long long (&s)[W], int C, int tpr, int sub, double M) {
  double e = 0.0;
#pragma unroll 1
  for (int k = 0; k * tpr < C; ++k) {
    const int c = k * tpr + sub;
    unsigned long long v = 0ull;
#pragma unroll
    for (int j = 0; j < W; ++j) v = j == c ? s[j] : v;
    double h = 0.0;  // h(0) = +0.0; h(1) = -0.0, lost in the sum
    if (v != 0ull) {
      const double p = __ddiv_rn(static_cast<double>(v), M);
      h = __dmul_rn(-p, log2(p));
    }
    for (int j = 0; j < tpr && k * tpr + j < C; ++j) e = __dadd_rn(e, __shfl(h, j, tpr));  // one rounding per add
  }
  return e;
}

// The row leader's epilogue: s holds the row's C class sums, entropy the
// row's class entropy (DAL_SOFT_ENTROPY only; DW: always).  DW: dens_pre, the
// row's density word, loaded with its flags.
// BALD: hs, the row's sum of leaf entropy words.
template <int W, bool DW, bool POW, bool BALD, class Args>
__device__ __forceinline__ void soft_epilogue(const Args& A, const unsigned long long (&s)[W], int64_t row,
                                              uint8_t fl, long long dens_pre, double M, double entropy,
                                              unsigned long long hs) {
  const int C = A.n_classes;
  // largest and second-largest sum, the lowest class holding the largest
  long long m1 = -1, m2 = -1;
  int arg = 0;
#pragma unroll
  for (int c = 0; c < W; ++c) {
    if (c < C) {
      const long long sc = static_cast<long long>(s[c]);
      if (sc > m1) {
        m2 = m1;
        m1 = sc;
        arg = c;
      } else if (sc > m2) {
        m2 = sc;
      }
    }
  }
  double score = entropy;  // DW: times density^beta below
  if constexpr (BALD) {
    // entropy - hsum / (T 2^29): one division of two exact doubles (hs < 2^41),
    // one subtraction; what the word rounding and the log2 push below zero
    // (and -0.0) is +0.0
    const double g = __ddiv_rn(static_cast<double>(hs), static_cast<double>(A.n_trees) *
                                                            static_cast<double>(1u << DAL_SOFT_ENTROPY_SHIFT));
    const double b = __dsub_rn(entropy, g);
    score = b > 0.0 ? b : 0.0;
    if (A.hsum) A.hsum[row] = hs;
    if (A.entropy) A.entropy[row] = entropy;
  } else if constexpr (!DW) {
    score = A.kind == DAL_SOFT_ENTROPY
                ? entropy
                : __ddiv_rn(static_cast<double>(A.kind == DAL_SOFT_MARGIN ? m1 - m2 : m1), M);
  }
  if (A.sums) {
    unsigned long long* sr = A.sums + row * C;
#pragma unroll
    for (int c = 0; c < W; ++c)
      if (c < C) sr[c] = s[c];
  }
  if (A.pred) A.pred[row] = static_cast<uint8_t>(arg);
  if constexpr (DW) {
    // the hard-vote kernels' density epilogue (forest_shared.hpp) on the class
    // entropy e (never NaN, >= +0.0): score = e d^beta, descending, and for
    // the GEMM density the interval score -+ e err(d^beta) as two keys
    const double e = entropy;
    double d = A.dkind == DAL_DENSITY_FIXED ? from_fixed(dens_pre) : __builtin_bit_cast(double, dens_pre);
    if (fl & DAL_ROW_EXCLUDED) d = __builtin_nan("");
    score = e * density_pow_if<POW>(d, A.beta);
    double err = 0.0;
    if (A.dkind == DAL_DENSITY_FIXED && e != 0.0 && d == d) {
      err = e * density_pow_err_if<POW>(d, A.derr, A.beta);
      // keep the interval ends distinct from the score after rounding
      err = fmax(err, fabs(score) * 4.5e-16);
    }
    unsigned long long klo = DAL_KEY_NONE, khi = DAL_KEY_NONE;
    if (fl & DAL_ROW_CANDIDATE) {
      klo = score_key(pessimistic(score, err, DAL_DESCENDING), DAL_DESCENDING);
      khi = score_key(optimistic(score, err, DAL_DESCENDING), DAL_DESCENDING);
    }
    A.entropy[row] = e;
    A.row_index[row] = static_cast<int32_t>(row);  // (n <= INT32_MAX, checked by the entry)
    A.scores[row] = score;
    A.keys[row] = klo;
    if (A.keys_hi) A.keys_hi[row] = khi;
  } else {
    A.scores[row] = score;
    A.keys[row] = (fl & DAL_ROW_CANDIDATE) ? score_key(score, A.order) : DAL_KEY_NONE;
  }
}

// Sums, prediction, score and key of tile `tile` (R rows from LDS or global
// memory): the walks, the cross-lane integer sum, then the row leader's
// epilogue.  fl_pre: the row leader's flags, loaded with the tile; DW:
// dens_pre, its density word, loaded with them (the epilogue's fp64
// temporaries exist on the row leader after the cross-lane sum only).  qstride:
// words per leaf row of leaf_q (the LDS copy's padded row, or C).
// BALD: leaf_h, the caller's entropy words (read when the forest is not in LDS).
template <int W, bool X_LDS, bool F_LDS, bool DW, bool POW, bool BALD, class Args>
__device__ __forceinline__ void score_tile_soft(const Args& A, const float* xs, int xstride, int64_t tile, int R,
                                                int tpr, const int2* inner, const int32_t* leaf_id,
                                                const uint32_t* leaf_q, int qstride, uint8_t fl_pre,
                                                long long dens_pre, const uint32_t* leaf_h) {
  const int n_inner = (1 << A.depth) - 1;
  const int n_leaf = 1 << A.depth;
  const int tid = threadIdx.x;
  const int r = tid / tpr;
  const int sub = tid - r * tpr;
  const int64_t row = tile * R + r;
  const bool live = r < R && row < A.n;
  const float* xrow = X_LDS ? xs + r * xstride : A.x + (live ? row : 0) * A.ldx;
  const unsigned last_leaf = static_cast<unsigned>(A.n_leaves - 1);

  unsigned long long s[W];
#pragma unroll
  for (int c = 0; c < W; ++c) s[c] = 0ull;
  unsigned long long hs = 0ull;  // BALD: the sum of the reached leaves' entropy words
  if (live) {
    int t = sub;
    for (; t + (kSoftIlp - 1) * tpr < A.n_trees; t += kSoftIlp * tpr) {
      int h[kSoftIlp];
#pragma unroll
      for (int j = 0; j < kSoftIlp; ++j) h[j] = 0;
      for (int lvl = 0; lvl < A.depth; ++lvl) {
#pragma unroll
        for (int j = 0; j < kSoftIlp; ++j) {
          const int2 nd = inner[(t + j * tpr) * n_inner + h[j]];
          const float xv = xrow[nd.x];
          h[j] = 2 * h[j] + (xv <= __int_as_float(nd.y) ? 1 : 2);
        }
      }
      unsigned l[kSoftIlp];
#pragma unroll
      for (int j = 0; j < kSoftIlp; ++j) {
        // (an id outside [0, n_leaves) is the caller's error: clamped, never read out of bounds)
        const unsigned id = static_cast<unsigned>(leaf_id[(t + j * tpr) * n_leaf + (h[j] - n_inner)]);
        l[j] = id < last_leaf ? id : last_leaf;
      }
#pragma unroll
      for (int j = 0; j < kSoftIlp; ++j) {
        const uint32_t* q = leaf_q + static_cast<size_t>(l[j]) * qstride;
        if constexpr (BALD) add_leaf_bald<W, F_LDS>(s, hs, q, A.n_classes, leaf_h, l[j]);
        else add_leaf<W, F_LDS>(s, q, A.n_classes);
      }
    }
    for (; t < A.n_trees; t += tpr) {
      int h = 0;
      for (int lvl = 0; lvl < A.depth; ++lvl) {
        const int2 nd = inner[t * n_inner + h];
        h = 2 * h + (xrow[nd.x] <= __int_as_float(nd.y) ? 1 : 2);
      }
      const unsigned id = static_cast<unsigned>(leaf_id[t * n_leaf + (h - n_inner)]);
      const unsigned l = id < last_leaf ? id : last_leaf;
      const uint32_t* q = leaf_q + static_cast<size_t>(l) * qstride;
      if constexpr (BALD) add_leaf_bald<W, F_LDS>(s, hs, q, A.n_classes, leaf_h, l);
      else add_leaf<W, F_LDS>(s, q, A.n_classes);
    }
  }
  // a row's tpr threads are consecutive lanes (tpr a power of two <= 64): their
  // partial sums add as integers, so the lane mapping cannot change a bit
  if constexpr (BALD) {  // (first: only the row leader reads it again, after the entropy)
    for (int o = 1; o < tpr; o <<= 1) hs += __shfl_xor(hs, o);
  }
  for (int o = 1; o < tpr; o <<= 1) {
#pragma unroll
    for (int c = 0; c < W; ++c) s[c] += __shfl_xor(s[c], o);
  }
  if constexpr (BALD && F_LDS) {
    // odd C: the entropy words went into s[C] with the 8-byte reads and were
    // added across the lanes with the class sums (hs is zero); s[C] is read by
    // nothing else (the entropy, the prediction and the stores stop at C)
    if (A.n_classes & 1) hs = soft_spare_sum<W>(s, A.n_classes);
  }
  const double M = static_cast<double>(A.n_trees) * 2147483648.0;  // T 2^31, exact
  double entropy = 0.0;
  if (DW || BALD || A.kind == DAL_SOFT_ENTROPY) entropy = soft_entropy<W>(s, A.n_classes, tpr, sub, M);  // (block-uniform)
  if (!(live && sub == 0)) return;
  soft_epilogue<W, DW, POW, BALD>(A, s, row, fl_pre, dens_pre, M, entropy, hs);
}

// What the body (forest_soft_body.inc) does for the density-weighted form
// alone, on its argument struct (nothing for SoftArgs): the step's status
// reset by the grid's first thread, and a row's density word.
template <bool DW, class Args>
__device__ __forceinline__ void soft_reset_status(const Args& A) {
  if constexpr (DW) {
    if (A.status_reset && blockIdx.x == 0 && threadIdx.x == 0) *A.status_reset = 0;
  }
}
template <bool DW, class Args>
__device__ __forceinline__ long long soft_density_word(const Args& A, int64_t row) {
  if constexpr (DW) return static_cast<const long long*>(A.density)[row];
  else return 0;
}

// One block per tile (grid = tiles), or PERSIST (LDS-DMA staging only; grid =
// the blocks resident at once, walking tiles blockIdx.x, + gridDim.x, ...): the
// forest is copied into LDS once per block instead of once per tile.
// LDS: [R staged rows | forest nodes | leaf ids | leaf table from the next 16-B boundary].
template <int W, bool X_LDS, bool F_LDS, bool PERSIST>
__global__ __launch_bounds__(kSoftThreads) void forest_soft_kernel(SoftArgs A, int R, int tpr, int x_floats, bool vec4,
                                                                   bool pad4, bool dma, int64_t n_tiles) {
  constexpr bool DW = false, POW = false, BALD = false;
#include "forest_soft_body.inc"
}

// The density-weighted form (dal_forest_score_soft_dw, dal_dw_step_soft): the
// same body, the density epilogue on the row leader.
template <int W, bool X_LDS, bool F_LDS, bool PERSIST, bool POW>
__global__ __launch_bounds__(kSoftThreads) void forest_soft_dw_kernel(SoftDwArgs A, int R, int tpr, int x_floats,
                                                                      bool vec4, bool pad4, bool dma,
                                                                      int64_t n_tiles) {
  constexpr bool DW = true, BALD = false;
#include "forest_soft_body.inc"
}

// The BALD form (dal_forest_score_soft_bald): the same body, one more integer
// accumulator per lane and the leaf's entropy word in its LDS row.
template <int W, bool X_LDS, bool F_LDS, bool PERSIST>
__global__ __launch_bounds__(kSoftThreads) void forest_soft_bald_kernel(SoftBaldArgs A, int R, int tpr, int x_floats,
                                                                        bool vec4, bool pad4, bool dma,
                                                                        int64_t n_tiles) {
  constexpr bool DW = false, POW = false, BALD = true;
#include "forest_soft_body.inc"
}

// The kernel of a form.
template <int W, bool XL, bool FL, bool PS, bool DW, bool POW, bool BALD>
constexpr auto soft_kernel() {
  if constexpr (BALD) return &forest_soft_bald_kernel<W, XL, FL, PS>;
  else if constexpr (DW) return &forest_soft_dw_kernel<W, XL, FL, PS, POW>;
  else return &forest_soft_kernel<W, XL, FL, PS>;
}

// The row-major tiling rule of the hard-vote kernels (forest_shared.hpp,
// forest_tiling).  DW (Args = SoftDwArgs): the density-weighted kernels, POW
// picked by beta -- the beta == 1 kernels hold no pow call.  BALD (Args =
// SoftBaldArgs): the residency test counts the leaf rows with the entropy
// word, so an even-C forest can leave LDS earlier than it does for the entropy.
template <int W, bool DW, bool POW, bool BALD, class Args>
int soft_launch(const Args& A, int64_t d, int64_t ldx, hipStream_t st) {
  const ForestTiling T = forest_tiling(A.x, d, ldx, A.n_trees, kSoftThreads);
  const int R = T.R, tpr = kSoftThreads / R;
  const int64_t blocks = ceil_div(A.n, R);
  const bool vec4 = (d % 4 == 0) && (ldx % 4 == 0) && (reinterpret_cast<uintptr_t>(A.x) % 16 == 0);
  const bool pad4 = vec4;
  const int xf = T.x_lds ? static_cast<int>(round_up(static_cast<int64_t>(R) * (d + (pad4 ? 4 : 1)), 4)) : 0;
  const int64_t n_inner = (int64_t{1} << A.depth) - 1, n_leaf = int64_t{1} << A.depth;
  // nodes, leaf ids, then the padded leaf table from the next 16-B boundary
  const int64_t f_bytes = round_up(A.n_trees * (n_inner * 8 + n_leaf * 4), 16) +
                          static_cast<int64_t>(A.n_leaves) * soft_lds_row<BALD>(A.n_classes) * 4;
  const bool f_lds = f_bytes <= kSoftForestLds;
  const size_t smem = static_cast<size_t>(xf) * 4 + (f_lds ? static_cast<size_t>(f_bytes) : 0);
#define DAL_SOFT_LAUNCH(XL, FL, PS)                                                                          \
  do {                                                                                                       \
    const auto kern = soft_kernel<W, XL, FL, PS, DW, POW, BALD>();                                           \
    const void* fn = reinterpret_cast<const void*>(kern);                                                    \
    int64_t grid = blocks;                                                                                   \
    if (PS) { /* a persistent grid of exactly the blocks resident at once */                                 \
      grid = persistent_grid(fn, kSoftThreads, smem, 0, blocks);                                             \
      if (grid < 0) return static_cast<int>(grid);                                                           \
    } else if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,                           \
                                   static_cast<int>(smem)) != hipSuccess) {                                  \
      return DAL_ERR_HIP;                                                                                    \
    }                                                                                                        \
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(kSoftThreads), smem, st, A, R, tpr, xf, \
                       vec4, pad4, T.dma, blocks);                                                           \
  } while (0)
  if (T.dma && f_lds) DAL_SOFT_LAUNCH(true, true, true);
  else if (T.dma) DAL_SOFT_LAUNCH(true, false, true);
  else if (T.x_lds && f_lds) DAL_SOFT_LAUNCH(true, true, false);
  else if (T.x_lds) DAL_SOFT_LAUNCH(true, false, false);
  else if (f_lds) DAL_SOFT_LAUNCH(false, true, false);
  else DAL_SOFT_LAUNCH(false, false, false);
#undef DAL_SOFT_LAUNCH
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

// f(std::integral_constant<int, W>{}) for the accumulator width of n_classes.
template <class F>
int dispatch_soft_width(int32_t n_classes, F&& f) {
  if (n_classes <= 2) return f(std::integral_constant<int, 2>{});
  if (n_classes <= 4) return f(std::integral_constant<int, 4>{});
  if (n_classes <= 8) return f(std::integral_constant<int, 8>{});
  if (n_classes <= 16) return f(std::integral_constant<int, 16>{});
  return f(std::integral_constant<int, 32>{});
}

// What both soft-vote entries check, in the order they report it: DAL_ERR_ARG
// (args_ok: the entry's own null-operand and enum tests) before DAL_ERR_SHAPE
// before DAL_ERR_UNSUPPORTED.  index32: the entry writes int32 row indices.
int soft_validate(bool args_ok, int64_t n, int64_t d, int64_t x_stride, int64_t n_leaves, int32_t n_trees,
                  int32_t depth, int32_t n_classes, bool index32) {
  if (!args_ok) return DAL_ERR_ARG;
  if (n < 0 || d < 1 || x_stride < d || d > (int64_t{1} << 30) || n_leaves < 1 || n_leaves > kSoftMaxLeaves)
    return DAL_ERR_SHAPE;
  if (index32 && n > INT32_MAX) return DAL_ERR_SHAPE;  // row_index is int32 (dal_dw_select's vote type)
  if (depth < 1 || depth > DAL_SOFT_MAX_DEPTH) return DAL_ERR_UNSUPPORTED;
  if (n_classes < 2 || n_classes > DAL_SOFT_MAX_CLASSES) return DAL_ERR_UNSUPPORTED;
  if (n_trees < 1 || n_trees > DAL_SOFT_MAX_TREES) return DAL_ERR_UNSUPPORTED;
  return DAL_OK;
}

int soft_dw_launch(const SoftStepScore& S, const void* density, int density_kind, const uint8_t* row_flags,
                   double* scores, uint64_t* keys, uint64_t* keys_hi, int32_t* status_reset, hipStream_t st) {
  const SoftDwArgs A{{S.x, S.n, static_cast<int>(S.d), S.ldx, reinterpret_cast<const int2*>(S.inner), S.leaf_id,
                      S.leaf_q, static_cast<int>(S.n_leaves), S.n_trees, S.depth, S.n_classes, DAL_SOFT_ENTROPY,
                      row_flags, DAL_DESCENDING, reinterpret_cast<unsigned long long*>(S.sums), S.pred, scores, keys},
                     density, density_kind, S.density_err, S.beta, S.entropy, S.row_index, keys_hi, status_reset};
  return dispatch_soft_width(S.n_classes, [&](auto w) {
    constexpr int W = decltype(w)::value;
    return S.beta == 1.0 ? soft_launch<W, true, false, false>(A, S.d, S.ldx, st)  // no pow, no call
                         : soft_launch<W, true, true, false>(A, S.d, S.ldx, st);
  });
}

}  // namespace

int forest_soft_step_check(const SoftStepScore& S, bool args_ok) {
  args_ok = args_ok && S.x && S.inner && S.leaf_id && S.leaf_q && S.density_fixed && S.entropy && S.row_index;
  return soft_validate(args_ok, S.n, S.d, S.ldx, S.n_leaves, S.n_trees, S.depth, S.n_classes, true);
}

int forest_soft_rows_per_block(const float* x, int64_t d, int64_t ldx, int32_t n_trees) {
  return forest_tiling(x, d, ldx, n_trees, kSoftThreads).R;
}

int forest_soft_step_launch(const SoftStepScore& S, const uint8_t* row_flags, double* scores, uint64_t* keys,
                            uint64_t* keys_hi, const ForestStepHooks& hooks, hipStream_t st) {
  // the status hook alone: no plan flags and no group fold in the soft kernel
  if (hooks.gmin || hooks.base_flags) return DAL_ERR_ARG;
  if (S.n == 0) return DAL_OK;
  return soft_dw_launch(S, S.density_fixed, DAL_DENSITY_FIXED, row_flags, scores, keys, keys_hi, hooks.status_reset,
                        st);
}

}  // namespace dal

using namespace dal;

extern "C" int dal_forest_soft_max_depth(void) { return DAL_SOFT_MAX_DEPTH; }

extern "C" int dal_forest_score_soft(const float* x, int64_t n, int64_t d, int64_t x_stride, const int32_t* inner,
                                     const int32_t* leaf_id, const uint32_t* leaf_q, int64_t n_leaves,
                                     int32_t n_trees, int32_t depth, int32_t n_classes, int score_kind,
                                     const uint8_t* row_flags, int order, uint64_t* sums, uint8_t* pred,
                                     double* scores, uint64_t* keys, dal_stream_t stream) {
  const bool args_ok =
      x && inner && leaf_id && leaf_q && scores && keys && (order == DAL_ASCENDING || order == DAL_DESCENDING) &&
      (score_kind == DAL_SOFT_LEAST_CONFIDENCE || score_kind == DAL_SOFT_MARGIN || score_kind == DAL_SOFT_ENTROPY);
  if (const int rc = soft_validate(args_ok, n, d, x_stride, n_leaves, n_trees, depth, n_classes, false)) return rc;
  if (n == 0) return DAL_OK;
  const SoftArgs A{x,
                   n,
                   static_cast<int>(d),
                   x_stride,
                   reinterpret_cast<const int2*>(inner),
                   leaf_id,
                   leaf_q,
                   static_cast<int>(n_leaves),
                   n_trees,
                   depth,
                   n_classes,
                   score_kind,
                   row_flags,
                   order,
                   reinterpret_cast<unsigned long long*>(sums),
                   pred,
                   scores,
                   keys};
  const hipStream_t st = as_stream(stream);
  return dispatch_soft_width(n_classes, [&](auto w) {
    return soft_launch<decltype(w)::value, false, false, false>(A, d, x_stride, st);
  });
}

extern "C" int dal_forest_score_soft_dw(const float* x, int64_t n, int64_t d, int64_t x_stride, const int32_t* inner,
                                        const int32_t* leaf_id, const uint32_t* leaf_q, int64_t n_leaves,
                                        int32_t n_trees, int32_t depth, int32_t n_classes, const void* density,
                                        int density_kind, double density_err, const uint8_t* row_flags, double beta,
                                        uint64_t* sums, uint8_t* pred, double* entropy, int32_t* row_index,
                                        double* scores, uint64_t* keys, uint64_t* keys_hi, dal_stream_t stream) {
  const bool args_ok = x && inner && leaf_id && leaf_q && density && entropy && row_index && scores && keys &&
                       (density_kind == DAL_DENSITY_FIXED || density_kind == DAL_DENSITY_EXACT);
  if (const int rc = soft_validate(args_ok, n, d, x_stride, n_leaves, n_trees, depth, n_classes, true)) return rc;
  if (n == 0) return DAL_OK;
  const SoftStepScore S{x,     n,         d,       x_stride, inner, leaf_id, leaf_q,  n_leaves, n_trees,
                        depth, n_classes, nullptr, density_err, beta, sums,   pred,    entropy,  row_index};
  return soft_dw_launch(S, density, density_kind, row_flags, scores, keys, keys_hi, nullptr, as_stream(stream));
}

extern "C" int dal_forest_score_soft_bald(const float* x, int64_t n, int64_t d, int64_t x_stride,
                                          const int32_t* inner, const int32_t* leaf_id, const uint32_t* leaf_q,
                                          const uint32_t* leaf_h, int64_t n_leaves, int32_t n_trees, int32_t depth,
                                          int32_t n_classes, const uint8_t* row_flags, int order, uint64_t* sums,
                                          uint8_t* pred, uint64_t* hsum, double* entropy, double* scores,
                                          uint64_t* keys, dal_stream_t stream) {
  const bool args_ok = x && inner && leaf_id && leaf_q && leaf_h && scores && keys &&
                       (order == DAL_ASCENDING || order == DAL_DESCENDING);
  if (const int rc = soft_validate(args_ok, n, d, x_stride, n_leaves, n_trees, depth, n_classes, false)) return rc;
  if (n == 0) return DAL_OK;
  const SoftBaldArgs A{{x, n, static_cast<int>(d), x_stride, reinterpret_cast<const int2*>(inner), leaf_id, leaf_q,
                        static_cast<int>(n_leaves), n_trees, depth, n_classes, DAL_SOFT_ENTROPY, row_flags, order,
                        reinterpret_cast<unsigned long long*>(sums), pred, scores, keys},
                       leaf_h, reinterpret_cast<unsigned long long*>(hsum), entropy};
  const hipStream_t st = as_stream(stream);
  return dispatch_soft_width(n_classes, [&](auto w) {
    return soft_launch<decltype(w)::value, false, false, true>(A, d, x_stride, st);
  });
}
