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
// tiling rule, the grid sizing, the counters and the row epilogue are the one
// definition of forest_shared.hpp, which the binary kernels and the blocked
// multiclass kernels use too; the staging loops are this kernel's own (the
// forms of forest.hip's: inside a shared helper they compiled the binary
// kernels, which are held to the instructions they had, to other code).
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
#include "forest_shared.hpp"

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

// Counts, prediction, score and key of tile `tile` (R rows from LDS or global
// memory): the walks, the cross-lane sum, then the row leader's epilogue
// (forest_shared.hpp).  fl_pre: the row leader's flags, loaded with the tile;
// DW: dens_pre, its density word, loaded with them.  The launcher picks POW by
// beta: the beta == 1 kernels hold no pow call at all.
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
  row_epilogue<CW, DW, POW>(A, w, row, fl_pre, dens_pre, lut_s);
}

// One block per tile (grid = tiles), or PERSIST (LDS-DMA staging only; grid =
// the blocks resident at once, walking tiles blockIdx.x, + gridDim.x, ...): the
// forest and the LUT are copied into LDS once per block instead of once per
// tile.  LDS: [R staged rows | LUT, T + 1 doubles | forest nodes, leaves].
// The body is forest_multi_body.inc: the kernels below and the step form's
// (McStepArgs: the density-weighted form's arguments and the step hooks).
struct McStepArgs : McDwArgs {
  ForestStepHooks hooks;
};

template <int CW, bool X_LDS, bool F_LDS, bool PERSIST, bool DW, bool POW>
__global__ __launch_bounds__(kMcThreads) void forest_multi_kernel(std::conditional_t<DW, McDwArgs, McArgs> A, int R,
                                                                  int tpr, int x_floats, bool vec4, bool pad4,
                                                                  bool dma, int64_t n_tiles) {
  constexpr bool STEP = std::is_same_v<decltype(A), McStepArgs>;  // false
#include "forest_multi_body.inc"
}

// dal_dw_step_multiclass's row-major kernel: the density-weighted form with
// the status and flag hooks, the same body.
template <int CW, bool X_LDS, bool F_LDS, bool PERSIST, bool POW>
__global__ __launch_bounds__(kMcThreads) void forest_multi_step_kernel(McStepArgs A, int R, int tpr, int x_floats,
                                                                       bool vec4, bool pad4, bool dma,
                                                                       int64_t n_tiles) {
  constexpr bool DW = true, STEP = true;
#include "forest_multi_body.inc"
}

// The kernel of a form: STEP (Args = McStepArgs) the one with the step hooks.
template <int CW, bool XL, bool FL, bool PS, bool DW, bool POW, bool STEP>
constexpr auto mc_kernel() {
  if constexpr (STEP) return &forest_multi_step_kernel<CW, XL, FL, PS, POW>;
  else return &forest_multi_kernel<CW, XL, FL, PS, DW, POW>;
}

// The binary launcher's tiling rule (forest_shared.hpp, forest_tiling).
template <int CW, bool DW, bool POW, bool STEP = false, class Args>
int multi_launch(const Args& A, int64_t d, int64_t ldx, hipStream_t st) {
  const ForestTiling T = forest_tiling(A.x, d, ldx, A.n_trees, kMcThreads);
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
    const auto kern = mc_kernel<CW, XL, FL, PS, DW, POW, STEP>();                                          \
    const void* fn = reinterpret_cast<const void*>(kern);                                                  \
    int64_t grid = blocks;                                                                                 \
    if (PS) { /* a persistent grid of exactly the blocks resident at once */                               \
      grid = persistent_grid(fn, kMcThreads, smem, 0, blocks);                                             \
      if (grid < 0) return static_cast<int>(grid);                                                         \
    } else if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,                         \
                                   static_cast<int>(smem)) != hipSuccess) {                                \
      return DAL_ERR_HIP;                                                                                  \
    }                                                                                                      \
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(kMcThreads), smem, st, A, R, tpr, xf, \
                       vec4, pad4, T.dma, blocks);                                                         \
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

int forest_multiclass_step_launch_rowmajor(const McStepScore& S, const uint8_t* row_flags, double* scores,
                                           uint64_t* keys, uint64_t* keys_hi, const ForestStepHooks& hooks,
                                           hipStream_t st) {
  if (hooks.gmin) return DAL_ERR_ARG;  // no group fold in the row-major kernel
  if (S.n == 0) return DAL_OK;
  const McStepArgs A{{{S.x, S.n, static_cast<int>(S.d), S.ldx, reinterpret_cast<const int2*>(S.inner), S.leaf,
                       S.n_trees, S.depth, S.n_classes, S.lut, DAL_MC_ENTROPY, row_flags, DAL_DESCENDING, S.counts,
                       S.pred, scores, keys, mc_cstore(S.counts, S.n_classes)},
                      S.density_fixed, DAL_DENSITY_FIXED, S.density_err, S.beta, S.entropy, S.row_index, keys_hi},
                     hooks};
  return dispatch_cw(S.n_classes, [&](auto cw) {
    constexpr int CW = decltype(cw)::value;
    return S.beta == 1.0 ? multi_launch<CW, true, false, true>(A, S.d, S.ldx, st)
                         : multi_launch<CW, true, true, true>(A, S.d, S.ldx, st);
  });
}

}  // namespace dal

using namespace dal;

extern "C" int dal_forest_multiclass_max_classes(void) { return DAL_MC_MAX_CLASSES; }

extern "C" int dal_forest_score_multiclass(const float* x, int64_t n, int64_t d, int64_t ldx, const int32_t* inner,
                                           const uint8_t* leaf, int32_t n_trees, int32_t depth, int32_t n_classes,
                                           const double* lut, int score_kind, const uint8_t* row_flags, int order,
                                           uint8_t* counts, uint8_t* pred, double* scores, uint64_t* keys,
                                           dal_stream_t stream) {
  const bool args_ok = x && inner && leaf && lut && scores && keys && mc_uncertainty_enums_ok(order, score_kind);
  if (const int rc = mc_validate(args_ok, n, d, ldx, n_trees, depth, n_classes, false)) return rc;
  if (n == 0) return DAL_OK;
  const McArgs A{x,         n,   static_cast<int>(d), ldx,       reinterpret_cast<const int2*>(inner),
                 leaf,      n_trees, depth,           n_classes, lut,
                 score_kind, row_flags, order,        counts,    pred,
                 scores,    keys, mc_cstore(counts, n_classes)};
  const hipStream_t st = as_stream(stream);
  return dispatch_cw(n_classes,
                     [&](auto cw) { return multi_launch<decltype(cw)::value, false, false>(A, d, ldx, st); });
}

extern "C" int dal_forest_score_multiclass_dw(const float* x, int64_t n, int64_t d, int64_t ldx, const int32_t* inner,
                                              const uint8_t* leaf, int32_t n_trees, int32_t depth, int32_t n_classes,
                                              const double* lut, const void* density, int density_kind,
                                              double density_err, const uint8_t* row_flags, double beta,
                                              uint8_t* counts, uint8_t* pred, double* entropy, int32_t* row_index,
                                              double* scores, uint64_t* keys, uint64_t* keys_hi,
                                              dal_stream_t stream) {
  const bool args_ok = x && inner && leaf && lut && density && entropy && row_index && scores && keys &&
                       (density_kind == DAL_DENSITY_FIXED || density_kind == DAL_DENSITY_EXACT);
  if (const int rc = mc_validate(args_ok, n, d, ldx, n_trees, depth, n_classes, true)) return rc;
  if (n == 0) return DAL_OK;
  const McDwArgs A{{x,         n,    static_cast<int>(d), ldx,       reinterpret_cast<const int2*>(inner),
                    leaf,      n_trees, depth,            n_classes, lut,
                    DAL_MC_ENTROPY, row_flags, DAL_DESCENDING, counts, pred,
                    scores,    keys, mc_cstore(counts, n_classes)},
                   density, density_kind, density_err, beta, entropy, row_index, keys_hi};
  const hipStream_t st = as_stream(stream);
  return dispatch_cw(n_classes, [&](auto cw) {
    constexpr int CW = decltype(cw)::value;
    return beta == 1.0 ? multi_launch<CW, true, false>(A, d, ldx, st)  // no pow, no call
                       : multi_launch<CW, true, true>(A, d, ldx, st);
  });
}
