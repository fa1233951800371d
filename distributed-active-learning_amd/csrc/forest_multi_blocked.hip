// Multiclass forest votes over the pool's blocked feature-major copy: the
// C-class form of forest.hip's prepared blocked kernel (forest_blocked_kernel
// <NW, PREP = true>), for the warm steps of a multiclass loop.
//
// Reference: as forest_multi.hip -- the per-tree predict and vote sum of
// final_thesis/uncertainty_sampling.py:88-97 for a forest of C classes, and
// the e*d product of density_weighting.py:148-167 for the density-weighted
// form.  The outputs are dal_forest_score_multiclass's and
// dal_forest_score_multiclass_dw's, bit for bit.
//
// MI355X design.  From the binary blocked kernel, as it is: a persistent grid;
// the forest prepared once per (forest, d) by dal_forest_prepare copied into
// LDS once per block, with the score LUT (T + 1 doubles) behind it; per 64-row
// tile only the runs of the features the forest tests, staged by
// global_load_lds_dwordx4, four 256-B runs per instruction; the rows on the 64
// lanes of every wave and the trees dealt over the NW waves (4, or 8 when a
// block's LDS lets at most two blocks onto a CU); byte-addressed walks, a
// select and a shift-add per level.  From forest_multi.hip: the votes as
// packed 8-bit fields in CW words (CW = 1, 2, 4, 8 for C <= 4, 8, 16, 32; every
// word index a compile-time constant) and the row leader's epilogue, the same
// arithmetic in the same order.  New here is only the cross-wave sum: a row's
// NW partial word sets sit in different waves, so waves 1 .. NW - 1 store
// theirs to an LDS exchange region ((NW - 1) CW words per row, lane-major: no
// bank conflicts) and wave 0 adds them field by field -- plain 32-bit adds, a
// field's total <= T <= 255 -- and runs the epilogue with lane = row.
//
// Two block barriers per tile: after the tile's DMA wait, and after the
// partial words are stored.  None closes the tile: every walk of tile k is
// over before its exchange barrier, so the other waves may stage tile k + 1
// while wave 0 writes tile k's rows out, and the exchange region is written
// again only after tile k + 1's DMA barrier, which wave 0 reaches after it
// has read tile k's words.
//
// LDS: [tile, fu_max runs of 256 B | prepared payload: nodes, leaves, feature
// list | LUT, round2(T + 1) doubles | exchange, (NW - 1) CW 256-B rows].
//
// The kernels' body is forest_multi_blocked_body.inc, included into the kernels
// the four score entries launch and into the step kernel of
// dal_dw_step_multiclass (forest_multi_blocked_step_kernel: the density-weighted
// form with ForestStepHooks -- status reset, plan flags, and the tiles' minimum
// keys folded into the top-k's row groups by wave 0).
//
// The prepared layout, a tile's DMA instruction, the walks, the counters and
// the row epilogue are forest_shared.hpp's, the definitions forest.hip and
// forest_multi.hip use (these kernels compile from them to the instructions
// they had with private copies); the applicability rule is built on forest.hip's
// exported probe, so the two cannot drift apart.
#include "forest_shared.hpp"

namespace dal {
namespace {

constexpr int kMcbIlp = 4;      // independent tree walks in flight per lane
constexpr int kMcbPerCu = 5;    // blocks per CU at most (forest.hip, DAL_FOREST_BLOCKED_PER_CU)
constexpr int kMcbWaves = 4;
constexpr int kMcbWavesWide = 8;
#ifndef DAL_MCB_STAGE_WAVE0
#define DAL_MCB_STAGE_WAVE0 0
#endif
// Wave 0 takes a share of a tile's DMA instructions (1), or the other waves
// issue them all while wave 0 is still in the previous tile's epilogue (0).
// With its share wave 0 issued it only after that epilogue, and the whole block
// waited for those loads: config 4 (C = 10, T = 10) 221.8 -> 200.1 us, its
// density-weighted form 232.9 -> 227.3 us, config 2 12.06 -> 11.36 us, config 3
// 41.9 -> 41.8 us (the row-major kernel beside it 426 / 429 us in the two runs;
// profiles/multiclass/blocked_stage_wave0_summary.json holds the run with 1).
constexpr bool kMcbStageWave0 = DAL_MCB_STAGE_WAVE0 != 0;

// (forest_multi.hip's McArgs without x, ldx, inner and leaf: the kernel reads
// the blocked copy and the prepared forest)
struct McArgs {
  int64_t n;
  int d;
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

struct McDwArgs : McArgs {
  const void* density;  // int64 fixed point (DAL_DENSITY_FIXED) or fp64 bits (DAL_DENSITY_EXACT), one word per row
  int dkind;
  double derr;
  double beta;
  double* entropy;
  int32_t* row_index;
  uint64_t* keys_hi;  // nullable
};

// The step form's arguments (dal_dw_step_multiclass): the density-weighted
// form's and the step hooks (common.hpp), with the meaning forest.hip gives
// them.  The kernels without hooks take the structs they always took.
struct McStepArgs : McDwArgs {
  ForestStepHooks hooks;
};

#ifndef DAL_MCB_DEFER_FOLD
#define DAL_MCB_DEFER_FOLD 1
#endif
// The step kernel's atomic group fold (several tiles per group) is issued by
// thread 0 after the NEXT tile's DMA wait in the four-wave kernels (1), or at
// once in the epilogue everywhere (0).  The fused step's device span, us,
// at once / deferred in every kernel, 30 rounds each, beside the unfused pair
// of the same run (kernel, group_min_kernel, select): config 4 (2M x 256,
// T = 10, C = 10, four waves) 267.8 / 249.3 (pair 255.7 / 256.5); config 4 at
// T = 100 (eight waves) 703.5 / 789.7 (pair 715.6 / 716.5); config 3 (four
// waves) 68.8 / 68.6 (pair 69.2 / 69.0).  So: deferred where the block has four
// waves, at once where it has eight.
constexpr bool kMcbDeferFold = DAL_MCB_DEFER_FOLD != 0;

// A tile's wave minima awaiting their atomics (thread 0 of the step kernel).
struct McbFold {
  unsigned long long lo = DAL_KEY_NONE, hi = DAL_KEY_NONE;
  uint32_t g = 0;
  bool pending = false;
};
__device__ __forceinline__ void mcb_issue_fold(const ForestStepHooks& H, McbFold& f) {
  if (!f.pending) return;
  unsigned long long* lo_g = reinterpret_cast<unsigned long long*>(H.gmin) + f.g;
  if (f.lo != DAL_KEY_NONE) atomicMax(lo_g, ~f.lo);
  if (f.hi != DAL_KEY_NONE) atomicMax(lo_g + H.n_groups, ~f.hi);
  f.pending = false;
}

template <int NW, int CW, bool DW, bool POW>
__global__ __launch_bounds__(NW * 64) void forest_multi_blocked_kernel(std::conditional_t<DW, McDwArgs, McArgs> A,
                                                                       const float* __restrict__ xb,
                                                                       const unsigned char* __restrict__ prep,
                                                                       int fu_max, int64_t n_tiles) {
  constexpr bool STEP = std::is_same_v<decltype(A), McStepArgs>;  // false
#include "forest_multi_blocked_body.inc"
}

// dal_dw_step_multiclass's kernel: the density-weighted form with the step
// hooks, the same body.
template <int NW, int CW, bool POW>
__global__ __launch_bounds__(NW * 64) void forest_multi_blocked_step_kernel(McStepArgs A,
                                                                            const float* __restrict__ xb,
                                                                            const unsigned char* __restrict__ prep,
                                                                            int fu_max, int64_t n_tiles) {
  constexpr bool DW = true, STEP = true;
#include "forest_multi_blocked_body.inc"
}

// The applicability rule and the launch shape.  The prepared forest is
// dal_forest_prepare's, so the rule starts from forest.hip's: a buffer exists
// (dal_forest_blocked_rows), and fu_max = min(nodes, d) is its bound on the
// distinct features.  The block's LDS is the tile, the payload, the LUT and the
// exchange region, within the 96 KiB the binary rule allows itself; 8 waves
// when four-wave blocks fit at most two per CU (the binary rule's threshold).
struct McbPlan {
  int fu_max = 0;  // 0: the blocked kernel does not apply
  int nw = 0;
  size_t smem = 0;
};
McbPlan mcb_plan(int64_t d, int32_t n_trees, int32_t depth, int32_t n_classes) {
  McbPlan P;
  if (n_classes < 2 || n_classes > DAL_MC_MAX_CLASSES || n_trees < 1 || n_trees > DAL_MC_MAX_TREES) return P;
  if (!dal_forest_blocked_rows(d, n_trees, depth)) return P;
  const int64_t nodes = static_cast<int64_t>(n_trees) * ((int64_t{1} << depth) - 1);
  const int64_t fu = nodes < d ? nodes : d;
  const BlockedPrepLayout L = blocked_prep_layout(n_trees, depth, fu);
  const size_t base = static_cast<size_t>(fu) * kBlk * 4 + static_cast<size_t>(L.payload) +
                      static_cast<size_t>(round_up(n_trees + 1, 2)) * 8;
  const size_t row_bytes = static_cast<size_t>(mc_words(n_classes)) * kBlk * 4;  // one wave's partial words
  const bool wide = base + (kMcbWaves - 1) * row_bytes > (160u << 10) / 3;
  const int nw = wide ? kMcbWavesWide : kMcbWaves;
  const size_t smem = base + (nw - 1) * row_bytes;
  if (smem > 96 * 1024) return P;
  P.fu_max = static_cast<int>(fu);
  P.nw = nw;
  P.smem = smem;
  return P;
}

// The kernel of a form: STEP (Args = McStepArgs) the one with the step hooks.
template <int NW, int CW, bool DW, bool POW, bool STEP>
constexpr auto mcb_kernel() {
  if constexpr (STEP) return &forest_multi_blocked_step_kernel<NW, CW, POW>;
  else return &forest_multi_blocked_kernel<NW, CW, DW, POW>;
}

template <int CW, bool DW, bool POW, bool STEP = false, class Args>
int mcb_launch(const Args& A, const float* xb, const void* fprep, const McbPlan& P, hipStream_t st) {
  const int64_t tiles = ceil_div(A.n, kBlk);
  const bool wide = P.nw == kMcbWavesWide;
  const auto kern = wide ? mcb_kernel<kMcbWavesWide, CW, DW, POW, STEP>() : mcb_kernel<kMcbWaves, CW, DW, POW, STEP>();
  // a persistent grid of the blocks resident at once, kMcbPerCu per CU at
  // most: every block stages the forest once (forest.hip)
  const int64_t grid = persistent_grid(reinterpret_cast<const void*>(kern), P.nw * 64, P.smem, kMcbPerCu, tiles);
  if (grid < 0) return static_cast<int>(grid);
  const unsigned char* pb = static_cast<const unsigned char*>(fprep);
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(P.nw * 64), P.smem, st, A, xb, pb, P.fu_max,
                     tiles);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

// The row-major entries' validation up to n == 0 (mc_validate), then the
// blocked operands': DAL_OK means launch.
int mcb_validate(bool args_ok, const float* xb, const void* fprep, int64_t n, int64_t d, int64_t ldx, int32_t n_trees,
                 int32_t depth, int32_t n_classes, bool index32) {
  if (const int rc = mc_validate(args_ok, n, d, ldx, n_trees, depth, n_classes, index32)) return rc;
  if (reinterpret_cast<uintptr_t>(xb) % 16 != 0) return DAL_ERR_ARG;
  if (mcb_plan(d, n_trees, depth, n_classes).fu_max && (!fprep || reinterpret_cast<uintptr_t>(fprep) % 16 != 0))
    return DAL_ERR_ARG;
  return DAL_OK;
}

}  // namespace

// The score launch of dal_dw_step_multiclass (common.hpp): the blocked kernel
// with the step hooks when the step has a blocked copy and the rule applies,
// else forest_multi.hip's row-major one (status and flag hooks only).
bool forest_multiclass_step_blocked(const float* xb, int64_t d, int32_t n_trees, int32_t depth, int32_t n_classes) {
  return xb && mcb_plan(d, n_trees, depth, n_classes).fu_max;
}

static_assert(kMcStepRows == kBlk, "the step's row groups are the blocked kernel's tiles");

int forest_multiclass_step_shape_check(int64_t n, int64_t d, int32_t n_trees, int32_t depth, int32_t n_classes) {
  return mc_validate(true, n, d, d, n_trees, depth, n_classes, true);
}

int forest_multiclass_step_check(const McStepScore& S, bool args_ok) {
  args_ok = args_ok && S.x && S.inner && S.leaf && S.lut && S.density_fixed && S.entropy && S.row_index;
  if (!S.xb) return mc_validate(args_ok, S.n, S.d, S.ldx, S.n_trees, S.depth, S.n_classes, true);
  return mcb_validate(args_ok, S.xb, S.fprep, S.n, S.d, S.ldx, S.n_trees, S.depth, S.n_classes, true);
}

int forest_multiclass_step_launch(const McStepScore& S, const uint8_t* row_flags, double* scores, uint64_t* keys,
                                  uint64_t* keys_hi, const ForestStepHooks& hooks, hipStream_t st) {
  if (S.n == 0) return DAL_OK;
  if (!forest_multiclass_step_blocked(S.xb, S.d, S.n_trees, S.depth, S.n_classes))
    return forest_multiclass_step_launch_rowmajor(S, row_flags, scores, keys, keys_hi, hooks, st);
  // the row groups are whole tiles, and every group index lies below n_groups
  if (hooks.gmin &&
      (hooks.group_blocks < 1 || ceil_div(ceil_div(S.n, kBlk), hooks.group_blocks) != hooks.n_groups))
    return DAL_ERR_ARG;
  const McbPlan P = mcb_plan(S.d, S.n_trees, S.depth, S.n_classes);
  const McStepArgs A{{{S.n, static_cast<int>(S.d), S.n_trees, S.depth, S.n_classes, S.lut, DAL_MC_ENTROPY, row_flags,
                       DAL_DESCENDING, S.counts, S.pred, scores, keys, mc_cstore(S.counts, S.n_classes)},
                      S.density_fixed, DAL_DENSITY_FIXED, S.density_err, S.beta, S.entropy, S.row_index, keys_hi},
                     hooks};
  return dispatch_cw(S.n_classes, [&](auto cw) {
    constexpr int CW = decltype(cw)::value;
    return S.beta == 1.0 ? mcb_launch<CW, true, false, true>(A, S.xb, S.fprep, P, st)
                         : mcb_launch<CW, true, true, true>(A, S.xb, S.fprep, P, st);
  });
}

}  // namespace dal

using namespace dal;

extern "C" int dal_forest_multiclass_blocked_rows(int64_t d, int32_t n_trees, int32_t depth, int32_t n_classes) {
  return mcb_plan(d, n_trees, depth, n_classes).fu_max ? kBlk : 0;
}

extern "C" int dal_forest_score_multiclass_blocked(const float* x, const float* xb, const void* fprep, int64_t n,
                                                   int64_t d, int64_t ldx, const int32_t* inner, const uint8_t* leaf,
                                                   int32_t n_trees, int32_t depth, int32_t n_classes,
                                                   const double* lut, int score_kind, const uint8_t* row_flags,
                                                   int order, uint8_t* counts, uint8_t* pred, double* scores,
                                                   uint64_t* keys, dal_stream_t stream) {
  if (!xb)
    return dal_forest_score_multiclass(x, n, d, ldx, inner, leaf, n_trees, depth, n_classes, lut, score_kind,
                                       row_flags, order, counts, pred, scores, keys, stream);
  const bool args_ok = x && inner && leaf && lut && scores && keys && mc_uncertainty_enums_ok(order, score_kind);
  if (const int rc = mcb_validate(args_ok, xb, fprep, n, d, ldx, n_trees, depth, n_classes, false)) return rc;
  if (n == 0) return DAL_OK;
  const McbPlan P = mcb_plan(d, n_trees, depth, n_classes);
  if (!P.fu_max)
    return dal_forest_score_multiclass(x, n, d, ldx, inner, leaf, n_trees, depth, n_classes, lut, score_kind,
                                       row_flags, order, counts, pred, scores, keys, stream);
  const McArgs A{n,     static_cast<int>(d), n_trees, depth, n_classes, lut,  score_kind, row_flags,
                 order, counts,              pred,    scores, keys,     mc_cstore(counts, n_classes)};
  const hipStream_t st = as_stream(stream);
  return dispatch_cw(n_classes,
                     [&](auto cw) { return mcb_launch<decltype(cw)::value, false, false>(A, xb, fprep, P, st); });
}

extern "C" int dal_forest_score_multiclass_dw_blocked(const float* x, const float* xb, const void* fprep, int64_t n,
                                                      int64_t d, int64_t ldx, const int32_t* inner,
                                                      const uint8_t* leaf, int32_t n_trees, int32_t depth,
                                                      int32_t n_classes, const double* lut, const void* density,
                                                      int density_kind, double density_err,
                                                      const uint8_t* row_flags, double beta, uint8_t* counts,
                                                      uint8_t* pred, double* entropy, int32_t* row_index,
                                                      double* scores, uint64_t* keys, uint64_t* keys_hi,
                                                      dal_stream_t stream) {
  if (!xb)
    return dal_forest_score_multiclass_dw(x, n, d, ldx, inner, leaf, n_trees, depth, n_classes, lut, density,
                                          density_kind, density_err, row_flags, beta, counts, pred, entropy,
                                          row_index, scores, keys, keys_hi, stream);
  const bool args_ok = x && inner && leaf && lut && density && entropy && row_index && scores && keys &&
                       (density_kind == DAL_DENSITY_FIXED || density_kind == DAL_DENSITY_EXACT);
  if (const int rc = mcb_validate(args_ok, xb, fprep, n, d, ldx, n_trees, depth, n_classes, true)) return rc;
  if (n == 0) return DAL_OK;
  const McbPlan P = mcb_plan(d, n_trees, depth, n_classes);
  if (!P.fu_max)
    return dal_forest_score_multiclass_dw(x, n, d, ldx, inner, leaf, n_trees, depth, n_classes, lut, density,
                                          density_kind, density_err, row_flags, beta, counts, pred, entropy,
                                          row_index, scores, keys, keys_hi, stream);
  const McDwArgs A{{n, static_cast<int>(d), n_trees, depth, n_classes, lut, DAL_MC_ENTROPY, row_flags, DAL_DESCENDING,
                    counts, pred, scores, keys, mc_cstore(counts, n_classes)},
                   density, density_kind, density_err, beta, entropy, row_index, keys_hi};
  const hipStream_t st = as_stream(stream);
  return dispatch_cw(n_classes, [&](auto cw) {
    constexpr int CW = decltype(cw)::value;
    return beta == 1.0 ? mcb_launch<CW, true, false>(A, xb, fprep, P, st)  // no pow, no call
                       : mcb_launch<CW, true, true>(A, xb, fprep, P, st);
  });
}
