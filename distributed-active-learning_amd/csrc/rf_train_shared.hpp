// What the binary trainer (rf_train.hip) and the C-class trainer
// (rf_train_multi.hip) share: the per-tree node states, the argument block of
// the level kernels and the label-independent steps -- binning, the status
// reset and the heap finalize.  Their kernels live in rf_train.hip; the
// launchers below are the only way in from another translation unit.
#pragma once

#include <cstring>

#include "common.hpp"

namespace dal {

constexpr uint8_t kAbsent = 0, kOpen = 1, kLeaf = 2;

struct RfArgs {
  const uint8_t* bins;     // [n][d]
  const uint8_t* labels;   // [n]
  const int32_t* weights;  // [T][n]
  const int32_t* subsets;  // [T][n_inner][m]
  const float* thresholds;
  const int32_t* n_splits;
  int64_t n;
  int d, m, T, max_depth, hb, kmax;
  int min_instances;
  double min_gain;
  int32_t* node;       // [T][n] heap index at the previous level (-1 settled)
  uint8_t* status;     // [T][n_all]
  int32_t* split_f;    // [T][n_inner]
  int32_t* split_b;    // [T][n_inner]
  int32_t* hist;       // binary: [T][2^l][m][hb][2]; C classes: [T][2^l][m][C][hb], the current level
  int32_t* cls;        // [T][2^l][C], ending where hist begins (rf_at_level)
  int32_t* out_inner;  // [T][n_inner][2]
  uint8_t* out_leaf;   // [T][n_leaf]
};

// Workspace offsets (256-B aligned pieces) for C classes.  The class totals
// come right before the histogram and a level's totals are kept at the END of
// their piece, so totals + histogram of a level are one span of int32 (what a
// sharded fit sums over ranks: dal_rf_train_level_span).
struct RfLayout {
  size_t bins, node, status, split_f, split_b, cls, hist, red, total;
};

// red_bytes: per (tree, split node) scratch of the C-class split kernel's
// cross-wave reduction (0 for the binary trainer: one wave per node).
inline RfLayout rf_layout(int64_t n, int64_t d, int64_t T, int max_depth, int64_t m, int64_t hb, int64_t C,
                          int64_t red_bytes) {
  RfLayout L{};
  const int64_t n_inner = (int64_t{1} << max_depth) - 1;
  const int64_t split_nodes = int64_t{1} << (max_depth - 1);  // deepest level that is split
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += static_cast<size_t>(round_up(static_cast<int64_t>(bytes), 256));
    return at;
  };
  L.bins = take(static_cast<size_t>(n * d));
  L.node = take(static_cast<size_t>(T * n * 4));
  L.status = take(static_cast<size_t>(T * (2 * n_inner + 1)));
  L.split_f = take(static_cast<size_t>(T * n_inner * 4));
  L.split_b = take(static_cast<size_t>(T * n_inner * 4));
  L.cls = take(static_cast<size_t>(T * (n_inner + 1) * C * 4));
  L.hist = take(static_cast<size_t>(T * split_nodes * m * hb * C * 4));
  L.red = take(static_cast<size_t>(T * split_nodes * red_bytes));
  L.total = o;
  return L;
}

// The job descriptor of the level steps (DAL_RF_JOB_BYTES of caller memory,
// filled by a begin entry): what dal_rf_train* keep on their stack between
// the steps.  A.cls holds the END of the totals piece (== A.hist).
constexpr uint32_t kRfJobMagic = 0x524a4f42u;
enum RfJobKind : int32_t { kRfJobBinary = 1, kRfJobMulti = 2, kRfJobRegress = 3 };

struct RfJob {
  uint32_t magic;
  int32_t kind;
  int32_t C;
  int32_t reserved;
  unsigned char* red;  // the C-class split kernel's scratch (null: binary)
  RfArgs A;
};
static_assert(sizeof(RfJob) <= DAL_RF_JOB_BYTES, "DAL_RF_JOB_BYTES holds a classifier job");

// A job of `kind` read from caller memory (any alignment) and a level inside
// [0, max_depth]: DAL_OK, DAL_ERR_ARG (null / not such a job) or DAL_ERR_SHAPE.
template <class Job>
inline int rf_job_load(const void* job, int32_t kind, int32_t level, Job* J) {
  if (!job) return DAL_ERR_ARG;
  std::memcpy(J, job, sizeof(Job));
  if (J->magic != kRfJobMagic || J->kind != kind) return DAL_ERR_ARG;
  if (level < 0 || level > J->A.max_depth) return DAL_ERR_SHAPE;
  return DAL_OK;
}

// The level's view of the job's arguments: the totals [T][2^l][C] end where
// the histogram begins.  ints = elements of the level's span from A.cls on.
inline RfArgs rf_at_level(const RfJob& J, int level, int64_t* ints) {
  RfArgs A = J.A;
  const int64_t nodes = int64_t{1} << level;
  const int64_t cls_ints = A.T * nodes * J.C;
  const int64_t hist_ints = level < A.max_depth ? A.T * nodes * A.m * A.hb * J.C : 0;
  A.cls = A.hist - cls_ints;
  *ints = cls_ints + hist_ints;
  return A;
}

// The argument checks of a classifier fit of C classes over n >= min_n rows
// (dal_rf_train's, in its order), the workspace layout and the job: no HIP
// call.  x, labels and weights may be null for a job of no rows.
int rf_job_setup(RfJob* J, int32_t kind, int32_t C, int64_t red_bytes, const float* x, int64_t n, int64_t d,
                 int64_t ldx, const uint8_t* labels, const float* thresholds, const int32_t* n_splits,
                 int32_t num_splits, const int32_t* weights, const int32_t* feature_subsets, int32_t m,
                 int32_t n_trees, int32_t max_depth, int32_t min_instances, double min_info_gain,
                 int32_t* out_inner, uint8_t* out_leaf, void* ws, size_t ws_bytes, int64_t min_n);

// dal_rf_train_level_span / dal_rf_train_multiclass_level_span.
int rf_level_span(const void* job, int32_t kind, int32_t level, void** ptr, int32_t* elem_type, int64_t* count);

// bins[i][f] =#{thresholds_f < x[i][f]} into A.bins; then every tree's root
// open and every other node absent.  No rows (A.n == 0): the reset alone.
// DAL_OK or DAL_ERR_HIP.
int rf_launch_bin_and_reset(const float* x, int64_t ldx, const RfArgs& A, hipStream_t st);

// (feature, fp32 threshold bits) per inner node into A.out_inner from
// A.split_f / A.split_b; absent and leaf positions become (0, +inf).
int rf_launch_finalize(const RfArgs& A, hipStream_t st);

}  // namespace dal
