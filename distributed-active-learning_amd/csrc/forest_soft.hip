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
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"  // (the shared header's pow helpers: unused here)
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

// Words per leaf row of the LDS copy of the leaf table: C rounded up to even,
// so a row is 8-byte aligned and read in 8-byte pieces.
__host__ __device__ inline int soft_lds_stride(int n_classes) { return (n_classes + 1) & ~1; }

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
// row's class entropy (DAL_SOFT_ENTROPY only).
template <int W>
__device__ __forceinline__ void soft_epilogue(const SoftArgs& A, const unsigned long long (&s)[W], int64_t row,
                                              uint8_t fl, double M, double entropy) {
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
  const double score = A.kind == DAL_SOFT_ENTROPY
                           ? entropy
                           : __ddiv_rn(static_cast<double>(A.kind == DAL_SOFT_MARGIN ? m1 - m2 : m1), M);
  if (A.sums) {
    unsigned long long* sr = A.sums + row * C;
#pragma unroll
    for (int c = 0; c < W; ++c)
      if (c < C) sr[c] = s[c];
  }
  if (A.pred) A.pred[row] = static_cast<uint8_t>(arg);
  A.scores[row] = score;
  A.keys[row] = (fl & DAL_ROW_CANDIDATE) ? score_key(score, A.order) : DAL_KEY_NONE;
}

// Sums, prediction, score and key of tile `tile` (R rows from LDS or global
// memory): the walks, the cross-lane integer sum, then the row leader's
// epilogue.  fl_pre: the row leader's flags, loaded with the tile.  qstride:
// words per leaf row of leaf_q (the LDS copy's padded row, or C).
template <int W, bool X_LDS, bool F_LDS>
__device__ __forceinline__ void score_tile_soft(const SoftArgs& A, const float* xs, int xstride, int64_t tile, int R,
                                                int tpr, const int2* inner, const int32_t* leaf_id,
                                                const uint32_t* leaf_q, int qstride, uint8_t fl_pre) {
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
      for (int j = 0; j < kSoftIlp; ++j) add_leaf<W, F_LDS>(s, leaf_q + static_cast<size_t>(l[j]) * qstride, A.n_classes);
    }
    for (; t < A.n_trees; t += tpr) {
      int h = 0;
      for (int lvl = 0; lvl < A.depth; ++lvl) {
        const int2 nd = inner[t * n_inner + h];
        h = 2 * h + (xrow[nd.x] <= __int_as_float(nd.y) ? 1 : 2);
      }
      const unsigned id = static_cast<unsigned>(leaf_id[t * n_leaf + (h - n_inner)]);
      add_leaf<W, F_LDS>(s, leaf_q + static_cast<size_t>(id < last_leaf ? id : last_leaf) * qstride, A.n_classes);
    }
  }
  // a row's tpr threads are consecutive lanes (tpr a power of two <= 64): their
  // partial sums add as integers, so the lane mapping cannot change a bit
  for (int o = 1; o < tpr; o <<= 1) {
#pragma unroll
    for (int c = 0; c < W; ++c) s[c] += __shfl_xor(s[c], o);
  }
  const double M = static_cast<double>(A.n_trees) * 2147483648.0;  // T 2^31, exact
  double entropy = 0.0;
  if (A.kind == DAL_SOFT_ENTROPY) entropy = soft_entropy<W>(s, A.n_classes, tpr, sub, M);  // (block-uniform)
  if (!(live && sub == 0)) return;
  soft_epilogue<W>(A, s, row, fl_pre, M, entropy);
}

// One block per tile (grid = tiles), or PERSIST (LDS-DMA staging only; grid =
// the blocks resident at once, walking tiles blockIdx.x, + gridDim.x, ...): the
// forest is copied into LDS once per block instead of once per tile.
// LDS: [R staged rows | forest nodes | leaf ids | leaf table from the next 16-B boundary].
template <int W, bool X_LDS, bool F_LDS, bool PERSIST>
__global__ __launch_bounds__(kSoftThreads) void forest_soft_kernel(SoftArgs A, int R, int tpr, int x_floats, bool vec4,
                                                                   bool pad4, bool dma, int64_t n_tiles) {
  static_assert(!PERSIST || X_LDS, "the persistent form stages rows by LDS-DMA");
  if (PERSIST) {
    dma = true;
    vec4 = false;
    pad4 = true;
  }
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* xs = reinterpret_cast<float*>(smem);
  const int n_inner = (1 << A.depth) - 1;
  const int n_leaf = 1 << A.depth;
  const int2* inner = A.inner;
  const int32_t* leaf_id = A.leaf_id;
  const uint32_t* leaf_q = A.leaf_q;
  int qstride = A.n_classes;
  const int tid = threadIdx.x;
  if (F_LDS) {
    // (x_floats % 4 == 0: the nodes start 16-B aligned)
    int2* fs = reinterpret_cast<int2*>(smem + static_cast<size_t>(x_floats) * 4);
    int32_t* ls = reinterpret_cast<int32_t*>(fs + A.n_trees * n_inner);
    const size_t q_off = static_cast<size_t>(
        round_up(static_cast<int64_t>(x_floats) * 4 + static_cast<int64_t>(A.n_trees) * (n_inner * 8 + n_leaf * 4), 16));
    uint32_t* qs = reinterpret_cast<uint32_t*>(smem + q_off);
    qstride = soft_lds_stride(A.n_classes);
    for (int e = tid; e < A.n_trees * n_inner; e += kSoftThreads) fs[e] = A.inner[e];
    for (int e = tid; e < A.n_trees * n_leaf; e += kSoftThreads) ls[e] = A.leaf_id[e];
    for (int e = tid; e < A.n_leaves * qstride; e += kSoftThreads) {
      const int l = e / qstride, c = e - l * qstride;
      qs[e] = c < A.n_classes ? A.leaf_q[l * A.n_classes + c] : 0u;
    }
    inner = fs;
    leaf_id = ls;
    leaf_q = qs;
  }
  // row stride in LDS: d + 1 words for scalar staging; d + 4 with 16-B staging
  // (rows stay 16-B aligned, rows of a wave start 4 banks apart)
  const int xstride = A.d + (pad4 ? 4 : 1);
  const int r = tid / tpr;  // (the row / tree-phase mapping of score_tile_soft)
  const int sub = tid - r * tpr;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // block-uniform
    const int64_t row0 = tile * R;
    const int64_t row = row0 + r;
    const bool live = r < R && row < A.n;
    // the row leader's flags are loaded with the tile (one HBM latency per tile)
    uint8_t fl_pre = DAL_ROW_CANDIDATE;
    if (A.flags && live && sub == 0) fl_pre = A.flags[row];
    if (X_LDS) {
      const int rows_here = static_cast<int>(min(static_cast<int64_t>(R), A.n - row0));
      if (dma) {
        // LDS-DMA staging (d % 4 == 0, 16-B-aligned padded rows): one
        // global_load_lds_dwordx4 per 1 KiB of a row (the last piece with only
        // the lanes it needs), lane l's 16 B landing at M0 + 16 l
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        const int row_bytes = A.d * 4;
        for (int rr = wave; rr < rows_here; rr += kSoftThreads / 64) {
          const float* src = A.x + (row0 + rr) * A.ldx;
          for (int p = 0; p * 1024 < row_bytes; ++p) {
            typedef __attribute__((address_space(3))) float lds_float;
            const unsigned dst = __builtin_amdgcn_readfirstlane(
                static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_float*)(xs + rr * xstride + p * 256))));
            const unsigned voff = static_cast<unsigned>(p * 1024 + lane * 16);
            if (static_cast<int>(voff) < row_bytes) lds_dma_x4(voff, dst, src);
          }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else if (vec4) {
        // 16-B loads, kStageBatch per thread issued before any LDS write
        constexpr int kStageBatch = 8;
        const int q = A.d >> 2, total = rows_here * q;
        for (int e0 = 0; e0 < total; e0 += kSoftThreads * kStageBatch) {
          typedef float v4f __attribute__((ext_vector_type(4)));
          v4f v[kStageBatch];
#pragma unroll
          for (int j = 0; j < kStageBatch; ++j) {
            const int e = e0 + j * kSoftThreads + tid;
            if (e < total) {
              const int rr = e / q, c = e - rr * q;
              v[j] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(A.x + (row0 + rr) * A.ldx) + c);
            }
          }
#pragma unroll
          for (int j = 0; j < kStageBatch; ++j) {
            const int e = e0 + j * kSoftThreads + tid;
            if (e < total) {
              const int rr = e / q, c = e - rr * q;
              *reinterpret_cast<v4f*>(xs + rr * xstride + 4 * c) = v[j];  // (vec4 implies pad4: 16-B aligned rows)
            }
          }
        }
      } else {
        for (int e = tid; e < rows_here * A.d; e += kSoftThreads) {
          const int rr = e / A.d, c = e - rr * A.d;
          xs[rr * xstride + c] = A.x[(row0 + rr) * A.ldx + c];
        }
      }
    }
    __syncthreads();
    score_tile_soft<W, X_LDS, F_LDS>(A, xs, xstride, tile, R, tpr, inner, leaf_id, leaf_q, qstride, fl_pre);
    if (!PERSIST) break;
    __syncthreads();  // every wave done with the tile before the next one is staged
  }
}

// The row-major tiling rule of the hard-vote kernels (forest_shared.hpp,
// forest_tiling).
template <int W>
int soft_launch(const SoftArgs& A, int64_t d, int64_t ldx, hipStream_t st) {
  const ForestTiling T = forest_tiling(A.x, d, ldx, A.n_trees, kSoftThreads);
  const int R = T.R, tpr = kSoftThreads / R;
  const int64_t blocks = ceil_div(A.n, R);
  const bool vec4 = (d % 4 == 0) && (ldx % 4 == 0) && (reinterpret_cast<uintptr_t>(A.x) % 16 == 0);
  const bool pad4 = vec4;
  const int xf = T.x_lds ? static_cast<int>(round_up(static_cast<int64_t>(R) * (d + (pad4 ? 4 : 1)), 4)) : 0;
  const int64_t n_inner = (int64_t{1} << A.depth) - 1, n_leaf = int64_t{1} << A.depth;
  // nodes, leaf ids, then the padded leaf table from the next 16-B boundary
  const int64_t f_bytes = round_up(A.n_trees * (n_inner * 8 + n_leaf * 4), 16) +
                          static_cast<int64_t>(A.n_leaves) * soft_lds_stride(A.n_classes) * 4;
  const bool f_lds = f_bytes <= kSoftForestLds;
  const size_t smem = static_cast<size_t>(xf) * 4 + (f_lds ? static_cast<size_t>(f_bytes) : 0);
#define DAL_SOFT_LAUNCH(XL, FL, PS)                                                                          \
  do {                                                                                                       \
    const auto kern = &forest_soft_kernel<W, XL, FL, PS>;                                                    \
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

}  // namespace
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
  if (!args_ok) return DAL_ERR_ARG;
  if (n < 0 || d < 1 || x_stride < d || d > (int64_t{1} << 30) || n_leaves < 1 || n_leaves > kSoftMaxLeaves)
    return DAL_ERR_SHAPE;
  if (depth < 1 || depth > DAL_SOFT_MAX_DEPTH) return DAL_ERR_UNSUPPORTED;
  if (n_classes < 2 || n_classes > DAL_SOFT_MAX_CLASSES) return DAL_ERR_UNSUPPORTED;
  if (n_trees < 1 || n_trees > DAL_SOFT_MAX_TREES) return DAL_ERR_UNSUPPORTED;
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
  if (n_classes <= 2) return soft_launch<2>(A, d, x_stride, st);
  if (n_classes <= 4) return soft_launch<4>(A, d, x_stride, st);
  if (n_classes <= 8) return soft_launch<8>(A, d, x_stride, st);
  if (n_classes <= 16) return soft_launch<16>(A, d, x_stride, st);
  return soft_launch<32>(A, d, x_stride, st);
}
