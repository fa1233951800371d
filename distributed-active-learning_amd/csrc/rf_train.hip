// Random-forest training on the GPU.
//
// Reference: the per-iteration model fit
//   RandomForest.trainClassifier(train, numClasses=2, categoricalFeaturesInfo={},
//                                numTrees=T, featureSubsetStrategy="auto",
//                                impurity='gini', maxDepth=4, maxBins=32)
//   final_thesis/uncertainty_sampling.py:71-76, density_weighting.py:119-124
// whose arithmetic is Apache Spark 2.1.0 MLlib (not vendored).  Restated for
// continuous features and binary labels (oracle/rf_oracle.py holds the CPU
// restatement with the algorithm's steps):
//   * candidate thresholds per feature: findSplitsForContinuousFeature
//     (distinct sorted values; all of them if few, else the stride rule);
//   * bins: #{thresholds < x} (Arrays.binarySearch), split k: bin <= k left;
//   * level-wise growth: weighted class histograms per (node, feature, bin),
//     Gini gain in fp64 in MLlib's operation order, first maximum over the
//     node's features (subset order) and splits (index order), leaf when
//     gain <= 0 or at maxDepth, children preset as leaves when pure.
// The bootstrap weights (Poisson counts) and per-node feature subsets come in
// from the caller (MLlib draws them from JVM RNGs that cannot be reproduced),
// so the result is deterministic and comparable with the oracle bit for bit.
//
// MI355X design: the training set of an AL iteration is the labeled window
// (10..~10^4 rows) -- small, so the work is latency- not bandwidth-bound and
// the design minimises launches: one block per feature sorts its sample in
// LDS (bitonic) and emits the thresholds with block-wide first-index
// searches; per level ONE histogram kernel (route rows from the previous
// level's decision + integer LDS atomics, flushed once per block: weights are
// integers, so the histograms are exact and order-free) and ONE split kernel
// (per-series prefix sums in LDS, every (feature, split) gain in fp64,
// lexicographic first-max reduction).
//
// This file owns the label-independent steps every trainer reaches through
// rf_train_shared.hpp: the classifiers' begin step (checks, layout, job), fp32
// thresholds and binning, the status reset (the regressor's too) and the heap
// finalize.  The level kernels are rf_train_multi.hip's: the binary fit
// (dal_rf_train*) is its C-class fit at C = 2, under its own job kind.
#include "rf_train_device.hpp"

namespace dal {
namespace {

// Heap arrays of dal_forest_score: (feature, fp32 threshold bits) per inner
// node; absent / leaf positions become always-left (0, +inf) padding.
__global__ void rf_finalize_kernel(RfArgs A) {
  const int n_inner = (1 << A.max_depth) - 1;
  const int64_t total = static_cast<int64_t>(A.T) * n_inner;
  for (int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; e < total;
       e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int t = static_cast<int>(e / n_inner), h = static_cast<int>(e - static_cast<int64_t>(t) * n_inner);
    const uint8_t s = A.status[static_cast<int64_t>(t) * (2 * n_inner + 1) + h];
    const int f = s == kAbsent ? -1 : A.split_f[e];
    int2 out = make_int2(0, __float_as_int(__builtin_inff()));
    if (f >= 0) out = make_int2(f, __float_as_int(A.thresholds[static_cast<int64_t>(f) * DAL_RF_MAX_SPLITS +
                                                                A.split_b[e]]));
    reinterpret_cast<int2*>(A.out_inner)[e] = out;
  }
}

__global__ void rf_reset_kernel(uint8_t* status, int T, int64_t n_all) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < T) status[static_cast<int64_t>(t) * n_all] = kOpen;
}

}  // namespace

// root open, everything else absent
int rf_launch_reset(uint8_t* status, int T, int max_depth, hipStream_t st) {
  const int64_t n_all = (int64_t{2} << max_depth) - 1;
  if (hipMemsetAsync(status, 0, static_cast<size_t>(T) * n_all, st) != hipSuccess) return DAL_ERR_HIP;
  hipLaunchKernelGGL(rf_reset_kernel, dim3(static_cast<unsigned>(ceil_div(T, 256))), dim3(256), 0, st, status, T,
                     n_all);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

int rf_launch_bin_and_reset(const float* x, int64_t ldx, const RfArgs& A, hipStream_t st) {
  if (A.n > 0)
    if (const int rc = launch_bin(x, A.n, A.d, ldx, A.thresholds, A.n_splits, const_cast<uint8_t*>(A.bins), st))
      return rc;
  return rf_launch_reset(A.status, A.T, A.max_depth, st);
}

int rf_launch_finalize(const RfArgs& A, hipStream_t st) {
  const int64_t n_inner = (int64_t{1} << A.max_depth) - 1;
  hipLaunchKernelGGL(rf_finalize_kernel,
                     dim3(static_cast<unsigned>(std::min<int64_t>(ceil_div(A.T * n_inner, 256), 4096))), dim3(256),
                     0, st, A);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

int rf_classifier_begin(RfJob* J, void* job, int32_t kind, int32_t C, int64_t min_n, hipStream_t st,
                        const float* x, int64_t n, int64_t d, int64_t ldx, const uint8_t* labels,
                        const float* thresholds, const int32_t* n_splits, int32_t num_splits,
                        const int32_t* weights, const int32_t* feature_subsets, int32_t m, int32_t n_trees,
                        int32_t max_depth, int32_t min_instances, double min_info_gain, int32_t* out_inner,
                        uint8_t* out_leaf, void* ws, size_t ws_bytes) {
  if (!J || !thresholds || !n_splits || !feature_subsets || !out_inner || !out_leaf || !ws) return DAL_ERR_ARG;
  if ((n > 0 || min_n > 0) && (!x || !labels || !weights)) return DAL_ERR_ARG;  // an empty shard has no rows to point at
  if (n < min_n || d < 1 || ldx < d || n_trees < 1 || m < 1 || m > d) return DAL_ERR_SHAPE;
  if (max_depth < 1 || max_depth > DAL_RF_MAX_DEPTH) return DAL_ERR_UNSUPPORTED;
  if (C < 2 || C > DAL_MC_MAX_CLASSES) return DAL_ERR_UNSUPPORTED;  // as dal_forest_score_multiclass
  if (num_splits < 0 || num_splits >= DAL_RF_MAX_SPLITS) return DAL_ERR_SHAPE;
  const int hb = num_splits + 2;  // find_splits emits at most num_splits + 1 thresholds
  // the split kernel keeps one node's whole (slot, bin, class) histogram in LDS
  if (static_cast<int64_t>(m) * hb * C * 4 > DAL_RF_SPLIT_LDS_BYTES) return DAL_ERR_UNSUPPORTED;
  const RfLayout L = rf_layout(n * d, n, n_trees, max_depth, m, hb, C, 4, kRedBytes);
  if (ws_bytes < L.total || reinterpret_cast<uintptr_t>(ws) % 256) return DAL_ERR_SHAPE;
  unsigned char* w = static_cast<unsigned char*>(ws);
  *J = RfJob{};
  J->magic = kRfJobMagic;
  J->kind = kind;
  J->C = C;
  J->red = w + L.red;
  RfArgs& A = J->A;
  A.bins = w + L.bins;
  A.labels = labels;
  A.weights = weights;
  A.subsets = feature_subsets;
  A.thresholds = thresholds;
  A.n_splits = n_splits;
  A.n = n;
  A.d = static_cast<int>(d);
  A.m = m;
  A.T = n_trees;
  A.max_depth = max_depth;
  A.hb = hb;
  A.kmax = num_splits + 1;
  A.min_instances = min_instances;
  A.min_gain = min_info_gain;
  A.node = reinterpret_cast<int32_t*>(w + L.node);
  A.status = w + L.status;
  A.split_f = reinterpret_cast<int32_t*>(w + L.split_f);
  A.split_b = reinterpret_cast<int32_t*>(w + L.split_b);
  A.hist = reinterpret_cast<int32_t*>(w + L.hist);
  A.tot = A.hist;
  A.out_inner = out_inner;
  A.out_leaf = out_leaf;
  if (job) std::memcpy(job, J, sizeof *J);
  return rf_launch_bin_and_reset(x, ldx, A, st);
}

}  // namespace dal

using namespace dal;

extern "C" int dal_rf_find_splits(const float* x, int64_t n, int64_t d, int64_t ldx, const int64_t* sample_rows,
                                  int64_t n_sample, int32_t num_splits, float* thresholds, int32_t* n_splits,
                                  int32_t* dev_status, dal_stream_t stream) {
  if (!x || !thresholds || !n_splits || !dev_status) return DAL_ERR_ARG;
  if (n < 1 || d < 1 || ldx < d || n_sample < 1 || n_sample > DAL_RF_MAX_SPLIT_SAMPLE) return DAL_ERR_SHAPE;
  if (!sample_rows && n_sample > n) return DAL_ERR_SHAPE;
  if (num_splits < 0 || num_splits >= DAL_RF_MAX_SPLITS) return DAL_ERR_SHAPE;
  return launch_find_splits(x, n, d, ldx, sample_rows, n_sample, num_splits, thresholds, n_splits, dev_status,
                            as_stream(stream));
}
