// The host side of what the forest trainers share (rf_train_multi.hip, the
// classifiers; rf_train_regress.hip, regression): the node
// states, the classifiers' argument block and job, the workspace layout and a
// level's view of it, and the label-independent steps -- the classifiers'
// begin, fp32 binning, the status reset and the classifiers' heap finalize --
// whose code lives in rf_train.hip; the functions below are the only way to
// it from another translation unit.  The device side is rf_train_device.hpp.
#pragma once

#include <cstring>

#include "common.hpp"

namespace dal {

constexpr uint8_t kAbsent = 0, kOpen = 1, kLeaf = 2;

// The C-class and regression split kernels: a block of kSplitWaves waves per
// node, whose first-maximum exchange takes kRedBytes of workspace per node --
// kSplitWaves gains (fp64) then kSplitWaves pair indices (int32).
constexpr int kSplitThreads = 256;
constexpr int kSplitWaves = kSplitThreads / kWave;
constexpr int kRedBytes = 64;
// A histogram kernel keeps the level's totals + histogram in LDS while they
// fit this budget, else it adds to global memory.
constexpr int64_t kHistLdsBytes = 64 * 1024;

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
  int32_t* hist;       // [T][2^l][m][C][hb], the current level
  int32_t* tot;        // class totals [T][2^l][C], ending where hist begins (rf_at_level)
  int32_t* out_inner;  // [T][n_inner][2]
  uint8_t* out_leaf;   // [T][n_leaf]
};

// Workspace offsets (256-B aligned pieces) of a trainer whose cells are
// `words` words of word_bytes each: C int32 class counts, or the regressor's
// W int64 words.  The totals come right before the histogram and a level's
// totals are kept at the END of their piece, so totals + histogram of a level
// are one span of words (what a sharded fit sums over ranks: the level_span
// entries).  bins_bytes: the job's own binned rows (0: the caller's);
// red_bytes: per (tree, split node) scratch of the split kernel's cross-wave
// reduction.
struct RfLayout {
  size_t bins, node, status, split_f, split_b, tot, hist, red, total;
};

inline RfLayout rf_layout(int64_t bins_bytes, int64_t n, int64_t T, int max_depth, int64_t m, int64_t hb,
                          int64_t words, int64_t word_bytes, int64_t red_bytes) {
  RfLayout L{};
  const int64_t n_inner = (int64_t{1} << max_depth) - 1;
  const int64_t split_nodes = int64_t{1} << (max_depth - 1);  // deepest level that is split
  size_t o = 0;
  auto take = [&](int64_t bytes) {
    const size_t at = o;
    o += static_cast<size_t>(round_up(bytes, 256));
    return at;
  };
  L.bins = take(bins_bytes);
  L.node = take(T * n * 4);
  L.status = take(T * (2 * n_inner + 1));
  L.split_f = take(T * n_inner * 4);
  L.split_b = take(T * n_inner * 4);
  L.tot = take(T * (n_inner + 1) * words * word_bytes);
  L.hist = take(T * split_nodes * m * hb * words * word_bytes);
  L.red = take(T * split_nodes * red_bytes);
  L.total = o;
  return L;
}

// The job descriptor of the level steps (DAL_RF_JOB_BYTES of caller memory,
// filled by a begin entry): what dal_rf_train* keep on their stack between
// the steps.  A.tot holds the END of the totals piece (== A.hist).
constexpr uint32_t kRfJobMagic = 0x524a4f42u;
enum RfJobKind : int32_t { kRfJobBinary = 1, kRfJobMulti = 2, kRfJobRegress = 3 };

struct RfJob {
  uint32_t magic;
  int32_t kind;
  int32_t C;
  int32_t reserved;
  unsigned char* red;  // the split kernel's scratch
  RfArgs A;
  int64_t words() const { return C; }  // per cell
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

// The level's view of a job's arguments (RfJob, or the regressor's job): the
// totals [T][2^l][words] end where the histogram begins.  count = elements of
// the level's span from A.tot on.
template <class Job>
inline auto rf_at_level(const Job& J, int level, int64_t* count) {
  auto A = J.A;
  const int64_t nodes = int64_t{1} << level;
  const int64_t tot_words = A.T * nodes * J.words();
  const int64_t hist_words = level < A.max_depth ? A.T * nodes * A.m * A.hb * J.words() : 0;
  A.tot = A.hist - tot_words;
  *count = tot_words + hist_words;
  return A;
}

// A classifier's begin step: the argument checks of a fit of C classes over
// n >= min_n rows (dal_rf_train's, in its order), the workspace layout and the
// job *J, copied to the caller's descriptor `job` (nullable) before the first
// device call; then rf_launch_bin_and_reset.  x, labels and weights may be
// null for a job of no rows.
int rf_classifier_begin(RfJob* J, void* job, int32_t kind, int32_t C, int64_t min_n, hipStream_t st,
                        const float* x, int64_t n, int64_t d, int64_t ldx, const uint8_t* labels,
                        const float* thresholds, const int32_t* n_splits, int32_t num_splits,
                        const int32_t* weights, const int32_t* feature_subsets, int32_t m, int32_t n_trees,
                        int32_t max_depth, int32_t min_instances, double min_info_gain, int32_t* out_inner,
                        uint8_t* out_leaf, void* ws, size_t ws_bytes);

// Every tree's root open and every other node absent, for T trees of
// max_depth.  DAL_OK or DAL_ERR_HIP.
int rf_launch_reset(uint8_t* status, int T, int max_depth, hipStream_t st);

// bins[i][f] = #{thresholds_f < x[i][f]} into A.bins (no rows, A.n == 0: none),
// then rf_launch_reset.
int rf_launch_bin_and_reset(const float* x, int64_t ldx, const RfArgs& A, hipStream_t st);

// (feature, fp32 threshold bits) per inner node into A.out_inner from
// A.split_f / A.split_b; absent and leaf positions become (0, +inf).
int rf_launch_finalize(const RfArgs& A, hipStream_t st);

}  // namespace dal
