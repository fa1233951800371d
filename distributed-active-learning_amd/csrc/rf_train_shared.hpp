// What the binary trainer (rf_train.hip) and the C-class trainer
// (rf_train_multi.hip) share: the per-tree node states, the argument block of
// the level kernels and the label-independent steps -- binning, the status
// reset and the heap finalize.  Their kernels live in rf_train.hip; the
// launchers below are the only way in from another translation unit.
#pragma once

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
  int32_t* cls;        // [T][2^l][C]
  int32_t* out_inner;  // [T][n_inner][2]
  uint8_t* out_leaf;   // [T][n_leaf]
};

// Workspace offsets (256-B aligned pieces) for C classes.
struct RfLayout {
  size_t bins, node, status, split_f, split_b, hist, cls, red, total;
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
  L.hist = take(static_cast<size_t>(T * split_nodes * m * hb * C * 4));
  L.cls = take(static_cast<size_t>(T * (n_inner + 1) * C * 4));
  L.red = take(static_cast<size_t>(T * split_nodes * red_bytes));
  L.total = o;
  return L;
}

// bins[i][f] =#{thresholds_f < x[i][f]} into A.bins; then every tree's root
// open and every other node absent.  DAL_OK or DAL_ERR_HIP.
int rf_launch_bin_and_reset(const float* x, int64_t ldx, const RfArgs& A, hipStream_t st);

// (feature, fp32 threshold bits) per inner node into A.out_inner from
// A.split_f / A.split_b; absent and leaf positions become (0, +inf).
int rf_launch_finalize(const RfArgs& A, hipStream_t st);

}  // namespace dal
