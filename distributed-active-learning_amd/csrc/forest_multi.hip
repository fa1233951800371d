// Multiclass random-forest hard votes fused with the uncertainty score.
//
// Reference: the per-tree predict and vote sum of
// final_thesis/uncertainty_sampling.py:88-97 for a forest trained with
// numClasses = C (RandomForest.trainClassifier takes it; the sklearn/ scripts
// train on iris and car): n_c(i) = the number of trees whose leaf for row i is
// class c.  The three scores are the C-class forms of the uncertainty
// strategies ("K2 multiclass"): one fp64 table of T + 1 entries,
// indexed by the largest count (least confidence), by the largest minus the
// second-largest count (margin), or summed over the classes in class order
// (entropy) -- sequential fp64 adds, so the score is the same bits as the
// host's Python floats.
//
// MI355X design: the row-major binary kernel's (forest.hip) -- an HBM stream;
// a block stages R pool rows in LDS (LDS-DMA for wide aligned rows on a
// persistent grid, 16-B or scalar loads for narrow rows, rows from global
// memory when 16 of them exceed 64 KiB), the forest is LDS-resident when it
// fits 64 KiB, and tpr = 256 / R threads share a row, each walking every
// tpr-th tree with 4 traversals in flight.  What differs is the vote: a
// thread keeps the C class counts as packed 8-bit fields, four per 32-bit
// word, in CW words (CW = 1, 2, 4, 8 for C <= 4, 8, 16, 32; a template
// parameter, every word index a compile-time constant so the words stay in
// registers).  T <= 255, so no field carries, in a thread or after the
// cross-lane sum of a row's tpr partial words (plain 32-bit adds).  The
// staging code is a copy of forest.hip's, not shared: the binary kernels'
// code generation does not move.
//
// The density-weighted form (template parameter DW; dal_forest_score_
// multiclass_dw) is the C-class reading of density_weighting.py:148-167's e*d
// product: the same walk, counters and staging, and a row-leader epilogue that
// multiplies the class entropy by density^beta and writes the interval keys
// of the binary kernel's density mode, plus the row's entropy and its own
// index, so that dal_dw_select (lut = entropy, votes = index) re-ranks it
// unchanged.  The DW = false kernels are the code they were without it.
//
// These are the row-major kernels: the cold step's, and every step's when the
// pool has no blocked copy.  The warm steps' form over the blocked
// feature-major copy and the prepared forest is forest_multi_blocked.hip
// (dal_forest_score_multiclass_blocked / _dw_blocked; same outputs, bit for
// bit), which also falls back to the entries below.
#include <type_traits>

#include "common.hpp"

namespace dal {
namespace {

constexpr int kMcThreads = 256;
constexpr int kMcIlp = 4;  // independent tree walks in flight per lane

struct McArgs {
  const float* x;
  int64_t n;
  int d;
  int64_t ldx;
  const int2* inner;
  const uint8_t* leaf;
  int n_trees;
  int depth;
  int n_classes;
  const double* lut;
  int kind;
  const uint8_t* flags;
  int order;
  uint8_t* counts;
  uint8_t* pred;
  double* scores;
  uint64_t* keys;
  int cstore;  // bytes per store of a row's counts: 4, 2 or 1 (by C and the buffer's alignment)
};

// The density-weighted form (DW): the entropy score times density^beta with
// interval keys, as the binary kernel's density mode (forest.hip).  Its
// arguments extend McArgs, so the uncertainty form's kernels take the struct
// they always took.
struct McDwArgs : McArgs {
  const void* density;  // int64 fixed point (DAL_DENSITY_FIXED) or fp64 bits (DAL_DENSITY_EXACT), one word per row
  int dkind;
  double derr;
  double beta;
  double* entropy;
  int32_t* row_index;
  uint64_t* keys_hi;  // nullable
};

// Copies of forest.hip's helpers (not shared: the binary kernels' code
// generation does not move).  pow stays out of line, and the launcher picks
// the kernel by beta: the beta == 1 kernels (POW false) hold no call at all --
// a call that is never taken still cost them 1 % (config 4, T = 10) to 3 %
// (T = 100) and 8 bytes of scratch per lane.
__device__ __attribute__((noinline)) double mc_density_pow_general(double d, double beta) { return pow(d, beta); }
template <bool POW>
__device__ __forceinline__ double mc_density_pow(double d, double beta) {
  if constexpr (POW) return mc_density_pow_general(d, beta);
  return d;
}

// |d^beta - d'^beta| bound for |d - d'| <= derr.
__device__ __attribute__((noinline)) double mc_density_pow_err_general(double d, double derr, double beta) {
  const double p = pow(fabs(d), beta);
  const double hi = pow(fabs(d) + derr, beta);
  const double lo = pow(fmax(fabs(d) - derr, 0.0), beta);
  return fmax(fabs(hi - p), fabs(p - lo)) * (1.0 + 1e-12) + fabs(p) * 1e-14;
}
template <bool POW>
__device__ __forceinline__ double mc_density_pow_err(double d, double derr, double beta) {
  if constexpr (POW) return mc_density_pow_err_general(d, derr, beta);
  return derr;
}

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

// Counts, prediction, score and key of tile `tile` (R rows from LDS or global
// memory).  fl_pre: the row leader's flags, loaded with the tile; DW: dens_pre,
// its density word, loaded with them.
template <int CW, bool X_LDS, bool DW, bool POW, class Args>
__device__ __forceinline__ void score_tile_multi(const Args& A, const float* xs, int xstride, int64_t tile, int R,
                                                 int tpr, const int2* inner, const uint8_t* leaf, uint8_t fl_pre,
                                                 long long dens_pre, const double* lut_s) {
  const int n_inner = (1 << A.depth) - 1;
  const int n_leaf = 1 << A.depth;
  const int tid = threadIdx.x;
  const int r = tid / tpr;
  const int sub = tid - r * tpr;
  const int64_t row = tile * R + r;
  const bool live = r < R && row < A.n;
  const float* xrow = X_LDS ? xs + r * xstride : A.x + (live ? row : 0) * A.ldx;

  unsigned w[CW];
#pragma unroll
  for (int j = 0; j < CW; ++j) w[j] = 0u;
  if (live) {
    int t = sub;
    for (; t + (kMcIlp - 1) * tpr < A.n_trees; t += kMcIlp * tpr) {
      int h[kMcIlp];
#pragma unroll
      for (int j = 0; j < kMcIlp; ++j) h[j] = 0;
      for (int lvl = 0; lvl < A.depth; ++lvl) {
#pragma unroll
        for (int j = 0; j < kMcIlp; ++j) {
          const int2 nd = inner[(t + j * tpr) * n_inner + h[j]];
          const float xv = xrow[nd.x];
          h[j] = 2 * h[j] + (xv <= __int_as_float(nd.y) ? 1 : 2);
        }
      }
      unsigned c[kMcIlp];
#pragma unroll
      for (int j = 0; j < kMcIlp; ++j) c[j] = leaf[(t + j * tpr) * n_leaf + (h[j] - n_inner)];
#pragma unroll
      for (int j = 0; j < kMcIlp; ++j) add_vote<CW>(w, c[j]);
    }
    for (; t < A.n_trees; t += tpr) {
      int h = 0;
      for (int lvl = 0; lvl < A.depth; ++lvl) {
        const int2 nd = inner[t * n_inner + h];
        h = 2 * h + (xrow[nd.x] <= __int_as_float(nd.y) ? 1 : 2);
      }
      add_vote<CW>(w, leaf[t * n_leaf + (h - n_inner)]);
    }
  }
  // a row's tpr threads are consecutive lanes: their partial words add field
  // by field (a field's total <= T <= 255)
  for (int o = 1; o < tpr; o <<= 1) {
#pragma unroll
    for (int j = 0; j < CW; ++j) w[j] += __shfl_xor(w[j], o);
  }
  if (!(live && sub == 0)) return;
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
    s = e * mc_density_pow<POW>(d, A.beta);
    double err = 0.0;
    if (A.dkind == DAL_DENSITY_FIXED && e != 0.0 && d == d) {
      err = e * mc_density_pow_err<POW>(d, A.derr, A.beta);
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
  } else {
    A.scores[row] = s;
    A.keys[row] = (fl_pre & DAL_ROW_CANDIDATE) ? score_key(s, A.order) : DAL_KEY_NONE;
  }
}

// One block per tile (grid = tiles), or PERSIST (LDS-DMA staging only; grid =
// the blocks resident at once, walking tiles blockIdx.x, + gridDim.x, ...): the
// forest and the LUT are copied into LDS once per block instead of once per
// tile.  LDS: [R staged rows | LUT, T + 1 doubles | forest nodes, leaves].
template <int CW, bool X_LDS, bool F_LDS, bool PERSIST, bool DW, bool POW>
__global__ __launch_bounds__(kMcThreads) void forest_multi_kernel(std::conditional_t<DW, McDwArgs, McArgs> A, int R,
                                                                  int tpr, int x_floats, bool vec4, bool pad4,
                                                                  bool dma, int64_t n_tiles) {
  static_assert(!PERSIST || X_LDS, "the persistent form stages rows by LDS-DMA");
  if (PERSIST) {
    dma = true;
    vec4 = false;
    pad4 = true;
  }
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* xs = reinterpret_cast<float*>(smem);
  double* lut_s = reinterpret_cast<double*>(smem + static_cast<size_t>(x_floats) * 4);  // (x_floats % 4 == 0)
  const int n_inner = (1 << A.depth) - 1;
  const int n_leaf = 1 << A.depth;
  const int2* inner = A.inner;
  const uint8_t* leaf = A.leaf;
  const int tid = threadIdx.x;
  for (int i = tid; i <= A.n_trees; i += kMcThreads) lut_s[i] = A.lut[i];  // (read after the staging barrier)
  if (F_LDS) {
    int2* fs = reinterpret_cast<int2*>(lut_s + round_up(A.n_trees + 1, 2));
    uint8_t* ls = reinterpret_cast<uint8_t*>(fs + A.n_trees * n_inner);
    for (int e = tid; e < A.n_trees * n_inner; e += kMcThreads) fs[e] = A.inner[e];
    for (int e = tid; e < A.n_trees * n_leaf; e += kMcThreads) ls[e] = A.leaf[e];
    inner = fs;
    leaf = ls;
  }
  // row stride in LDS: d + 1 words for scalar staging; d + 4 with 16-B staging
  // (rows stay 16-B aligned, rows of a wave start 4 banks apart)
  const int xstride = A.d + (pad4 ? 4 : 1);
  const int r = tid / tpr;  // (the row / tree-phase mapping of score_tile_multi)
  const int sub = tid - r * tpr;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // block-uniform
    const int64_t row0 = tile * R;
    const int64_t row = row0 + r;
    const bool live = r < R && row < A.n;
    // the row leader's flags are loaded with the tile (one HBM latency per tile)
    uint8_t fl_pre = DAL_ROW_CANDIDATE;
    if (A.flags && live && sub == 0) fl_pre = A.flags[row];
    long long dens_pre = 0;  // ... and, DW, its density word
    if constexpr (DW) {
      if (live && sub == 0) dens_pre = static_cast<const long long*>(A.density)[row];
    }
    if (X_LDS) {
      const int rows_here = static_cast<int>(min(static_cast<int64_t>(R), A.n - row0));
      if (dma) {
        // LDS-DMA staging (d % 4 == 0, 16-B-aligned padded rows): one
        // global_load_lds_dwordx4 per 1 KiB of a row (the last piece with only
        // the lanes it needs), lane l's 16 B landing at M0 + 16 l
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        const int row_bytes = A.d * 4;
        for (int rr = wave; rr < rows_here; rr += kMcThreads / 64) {
          const float* src = A.x + (row0 + rr) * A.ldx;
          for (int p = 0; p * 1024 < row_bytes; ++p) {
            typedef __attribute__((address_space(3))) float lds_float;
            const unsigned dst = __builtin_amdgcn_readfirstlane(
                static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_float*)(xs + rr * xstride + p * 256))));
            const unsigned voff = static_cast<unsigned>(p * 1024 + lane * 16);
            if (static_cast<int>(voff) < row_bytes) {
              unsigned keep;
              asm volatile(
                  "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                  "global_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                  : "=&s"(keep)
                  : "v"(voff), "s"(dst), "s"(src)
                  : "memory");
            }
          }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else if (vec4) {
        // 16-B loads, kStageBatch per thread issued before any LDS write
        constexpr int kStageBatch = 8;
        const int q = A.d >> 2, total = rows_here * q;
        for (int e0 = 0; e0 < total; e0 += kMcThreads * kStageBatch) {
          typedef float v4f __attribute__((ext_vector_type(4)));
          v4f v[kStageBatch];
#pragma unroll
          for (int j = 0; j < kStageBatch; ++j) {
            const int e = e0 + j * kMcThreads + tid;
            if (e < total) {
              const int rr = e / q, c = e - rr * q;
              v[j] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(A.x + (row0 + rr) * A.ldx) + c);
            }
          }
#pragma unroll
          for (int j = 0; j < kStageBatch; ++j) {
            const int e = e0 + j * kMcThreads + tid;
            if (e < total) {
              const int rr = e / q, c = e - rr * q;
              *reinterpret_cast<v4f*>(xs + rr * xstride + 4 * c) = v[j];  // (vec4 implies pad4: 16-B aligned rows)
            }
          }
        }
      } else {
        for (int e = tid; e < rows_here * A.d; e += kMcThreads) {
          const int rr = e / A.d, c = e - rr * A.d;
          xs[rr * xstride + c] = A.x[(row0 + rr) * A.ldx + c];
        }
      }
    }
    __syncthreads();
    score_tile_multi<CW, X_LDS, DW, POW>(A, xs, xstride, tile, R, tpr, inner, leaf, fl_pre, dens_pre, lut_s);
    if (!PERSIST) break;
    __syncthreads();  // every wave done with the tile before the next one is staged
  }
}

struct McTiling {
  int R;       // rows per block
  bool x_lds;  // pool rows staged in LDS
  bool dma;    // ... by LDS-DMA (wide rows)
};

// The binary launcher's tiling rule (forest.hip, forest_tiling; the figures
// behind its thresholds are there): ~16 KiB tiles, 32 KiB with LDS-DMA
// (d >= 128, 16-B aligned rows), rows from global memory when 16 of them pass
// 64 KiB, and at least two lanes per row from 64 trees on.
McTiling multi_tiling(const float* x, int64_t d, int64_t ldx, int32_t n_trees) {
  McTiling T{256, true, false};
  T.dma = d >= 128 && d % 4 == 0 && ldx % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
  const int64_t tile_cap = T.dma ? 33280 : 16640;
  while (T.R > 16 && static_cast<int64_t>(T.R) * (d + 1) * 4 > tile_cap) T.R >>= 1;
  if (static_cast<int64_t>(T.R) * (d + 1) * 4 > 65536) {
    T.x_lds = false;
    T.dma = false;
    T.R = 256;
  }
  const int tpr_min = n_trees >= 64 ? 2 : 1;
  if (T.x_lds) {
    while (T.R > 1 && kMcThreads / T.R < tpr_min) T.R >>= 1;
  }
  return T;
}

template <int CW, bool DW, bool POW, class Args>
int multi_launch(const Args& A, const McTiling& T, int64_t d, int64_t ldx, hipStream_t st) {
  const int R = T.R, tpr = kMcThreads / R;
  const int64_t blocks = ceil_div(A.n, R);
  const bool vec4 = (d % 4 == 0) && (ldx % 4 == 0) && (reinterpret_cast<uintptr_t>(A.x) % 16 == 0);
  const bool pad4 = vec4;
  const int xf = T.x_lds ? static_cast<int>(round_up(static_cast<int64_t>(R) * (d + (pad4 ? 4 : 1)), 4)) : 0;
  const int64_t n_inner = (int64_t{1} << A.depth) - 1, n_leaf = int64_t{1} << A.depth;
  const int64_t f_bytes = A.n_trees * (n_inner * 8 + n_leaf);
  const bool f_lds = f_bytes <= 65536;
  const size_t smem = static_cast<size_t>(xf) * 4 + static_cast<size_t>(round_up(A.n_trees + 1, 2)) * 8 +
                      (f_lds ? static_cast<size_t>(f_bytes) : 0);
#define DAL_MC_LAUNCH(XL, FL, PS)                                                                          \
  do {                                                                                                     \
    const void* fn = reinterpret_cast<const void*>(forest_multi_kernel<CW, XL, FL, PS, DW, POW>);          \
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem)) !=     \
        hipSuccess)                                                                                        \
      return DAL_ERR_HIP;                                                                                  \
    int64_t grid = blocks;                                                                                 \
    if (PS) { /* a persistent grid of exactly the blocks resident at once */                               \
      int dev = 0, cus = 0, per_cu = 0;                                                                    \
      if (hipGetDevice(&dev) != hipSuccess ||                                                              \
          hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||         \
          cus < 1 || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kMcThreads, smem) != hipSuccess) \
        return DAL_ERR_HIP;                                                                                \
      if (per_cu < 1) per_cu = 1;                                                                          \
      if (grid > static_cast<int64_t>(cus) * per_cu) grid = static_cast<int64_t>(cus) * per_cu;            \
    }                                                                                                      \
    hipLaunchKernelGGL((forest_multi_kernel<CW, XL, FL, PS, DW, POW>), dim3(static_cast<unsigned>(grid)),  \
                       dim3(kMcThreads), smem, st, A, R, tpr, xf, vec4, pad4, T.dma, blocks);              \
  } while (0)
  if (T.dma && f_lds) DAL_MC_LAUNCH(true, true, true);
  else if (T.dma) DAL_MC_LAUNCH(true, false, true);
  else if (T.x_lds && f_lds) DAL_MC_LAUNCH(true, true, false);
  else if (T.x_lds) DAL_MC_LAUNCH(true, false, false);
  else if (f_lds) DAL_MC_LAUNCH(false, true, false);
  else DAL_MC_LAUNCH(false, false, false);
#undef DAL_MC_LAUNCH
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" int dal_forest_multiclass_max_classes(void) { return DAL_MC_MAX_CLASSES; }

extern "C" int dal_forest_score_multiclass(const float* x, int64_t n, int64_t d, int64_t ldx, const int32_t* inner,
                                           const uint8_t* leaf, int32_t n_trees, int32_t depth, int32_t n_classes,
                                           const double* lut, int score_kind, const uint8_t* row_flags, int order,
                                           uint8_t* counts, uint8_t* pred, double* scores, uint64_t* keys,
                                           dal_stream_t stream) {
  if (!x || !inner || !leaf || !lut || !scores || !keys) return DAL_ERR_ARG;
  if (order != DAL_ASCENDING && order != DAL_DESCENDING) return DAL_ERR_ARG;
  if (score_kind != DAL_MC_LEAST_CONFIDENCE && score_kind != DAL_MC_MARGIN && score_kind != DAL_MC_ENTROPY)
    return DAL_ERR_ARG;
  if (n < 0 || d < 1 || ldx < d || d > (int64_t{1} << 30)) return DAL_ERR_SHAPE;
  if (depth < 1 || depth > DAL_MAX_TREE_DEPTH) return DAL_ERR_UNSUPPORTED;
  if (n_classes < 2 || n_classes > DAL_MC_MAX_CLASSES) return DAL_ERR_UNSUPPORTED;
  if (n_trees < 1 || n_trees > DAL_MC_MAX_TREES) return DAL_ERR_UNSUPPORTED;
  if (n == 0) return DAL_OK;
  const uintptr_t ca = reinterpret_cast<uintptr_t>(counts);
  const int cstore = (n_classes % 4 == 0 && ca % 4 == 0) ? 4 : (n_classes % 2 == 0 && ca % 2 == 0) ? 2 : 1;
  const McArgs A{x,         n,   static_cast<int>(d), ldx,       reinterpret_cast<const int2*>(inner),
                 leaf,      n_trees, depth,           n_classes, lut,
                 score_kind, row_flags, order,        counts,    pred,
                 scores,    keys, cstore};
  const McTiling T = multi_tiling(x, d, ldx, n_trees);
  const hipStream_t st = as_stream(stream);
  if (n_classes <= 4) return multi_launch<1, false, false>(A, T, d, ldx, st);
  if (n_classes <= 8) return multi_launch<2, false, false>(A, T, d, ldx, st);
  if (n_classes <= 16) return multi_launch<4, false, false>(A, T, d, ldx, st);
  return multi_launch<8, false, false>(A, T, d, ldx, st);
}

extern "C" int dal_forest_score_multiclass_dw(const float* x, int64_t n, int64_t d, int64_t ldx, const int32_t* inner,
                                              const uint8_t* leaf, int32_t n_trees, int32_t depth, int32_t n_classes,
                                              const double* lut, const void* density, int density_kind,
                                              double density_err, const uint8_t* row_flags, double beta,
                                              uint8_t* counts, uint8_t* pred, double* entropy, int32_t* row_index,
                                              double* scores, uint64_t* keys, uint64_t* keys_hi,
                                              dal_stream_t stream) {
  if (!x || !inner || !leaf || !lut || !density || !entropy || !row_index || !scores || !keys) return DAL_ERR_ARG;
  if (density_kind != DAL_DENSITY_FIXED && density_kind != DAL_DENSITY_EXACT) return DAL_ERR_ARG;
  if (n < 0 || d < 1 || ldx < d || d > (int64_t{1} << 30)) return DAL_ERR_SHAPE;
  if (n > INT32_MAX) return DAL_ERR_SHAPE;  // row_index is int32 (dal_dw_select's vote type)
  if (depth < 1 || depth > DAL_MAX_TREE_DEPTH) return DAL_ERR_UNSUPPORTED;
  if (n_classes < 2 || n_classes > DAL_MC_MAX_CLASSES) return DAL_ERR_UNSUPPORTED;
  if (n_trees < 1 || n_trees > DAL_MC_MAX_TREES) return DAL_ERR_UNSUPPORTED;
  if (n == 0) return DAL_OK;
  const uintptr_t ca = reinterpret_cast<uintptr_t>(counts);
  const int cstore = (n_classes % 4 == 0 && ca % 4 == 0) ? 4 : (n_classes % 2 == 0 && ca % 2 == 0) ? 2 : 1;
  const McDwArgs A{{x,         n,    static_cast<int>(d), ldx,       reinterpret_cast<const int2*>(inner),
                    leaf,      n_trees, depth,            n_classes, lut,
                    DAL_MC_ENTROPY, row_flags, DAL_DESCENDING, counts, pred,
                    scores,    keys, cstore},
                   density, density_kind, density_err, beta, entropy, row_index, keys_hi};
  const McTiling T = multi_tiling(x, d, ldx, n_trees);
  const hipStream_t st = as_stream(stream);
  if (beta == 1.0) {  // no pow, no call
    if (n_classes <= 4) return multi_launch<1, true, false>(A, T, d, ldx, st);
    if (n_classes <= 8) return multi_launch<2, true, false>(A, T, d, ldx, st);
    if (n_classes <= 16) return multi_launch<4, true, false>(A, T, d, ldx, st);
    return multi_launch<8, true, false>(A, T, d, ldx, st);
  }
  if (n_classes <= 4) return multi_launch<1, true, true>(A, T, d, ldx, st);
  if (n_classes <= 8) return multi_launch<2, true, true>(A, T, d, ldx, st);
  if (n_classes <= 16) return multi_launch<4, true, true>(A, T, d, ldx, st);
  return multi_launch<8, true, true>(A, T, d, ldx, st);
}
