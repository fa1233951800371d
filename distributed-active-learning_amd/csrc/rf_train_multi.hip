// Random-forest training on the GPU for C classes (2 <= C <= DAL_MC_MAX_CLASSES):
//   RandomForest.trainClassifier(train, numClasses=C, categoricalFeaturesInfo={},
//                                numTrees=T, featureSubsetStrategy="auto",
//                                impurity='gini', maxDepth=4, maxBins=32)
//   final_thesis/uncertainty_sampling.py:71-76, density_weighting.py:119-124
// The algorithm is the one of rf_train.hip (its header comment has the steps)
// with C classes wherever two appear there, and the binary fit is this file's
// at C = 2 (dal_rf_train*: its own job kind, the same kernels -- at C = 2 the
// arithmetic below is the binary Gini's operation for operation).  This file
// owns the two level kernels and the Gini of C counts; the begin step, binning,
// the status reset and the heap finalize are rf_train.hip's
// (rf_train_shared.hpp), routing, prefix sums, the first-maximum reduction,
// the commit and the entry ladder are rf_train_device.hpp's.
//
//   histogram  [tree][node][slot][class][bin], bins innermost: the split
//              kernel's lanes take consecutive split indices k and so read
//              consecutive LDS words for each class (class innermost would put
//              them C words apart: a 32-way bank conflict at C = 32).
//   split      one block of 4 waves per node: the node's histogram is copied
//              to LDS, every (slot, class) series is prefix-summed in place
//              (m * C independent series), then every (slot, split) pair's
//              gain is computed in fp64 in MLlib's operation order -- total
//              from integers, imp = 1, imp -= f * f per class in class order
//              (a zero count leaves imp unchanged and is skipped), gain =
//              parent - (lc/tc) * imp_l - (rc/tc) * imp_r, no FMA -- and the
//              lexicographic first maximum (gain desc, pair index asc) is
//              reduced over the wave by shuffles and over the four waves
//              through 64 bytes of workspace per node (the LDS is the
//              histogram's up to its last byte).
#include "rf_train_device.hpp"

namespace dal {
namespace {

// Gini.calculate over C counts read through cnt(c); total = their sum.
template <class Counts>
__device__ __forceinline__ double gini_c(Counts cnt, int C, int64_t total_i) {
  if (total_i == 0) return 0.0;
  const double total = static_cast<double>(total_i);
  double imp = 1.0;
  for (int c = 0; c < C; ++c) {
    const int64_t v = cnt(c);
    if (v == 0) continue;  // f = 0: imp - 0 * 0 == imp
    const double f = static_cast<double>(v) / total;
    imp -= f * f;
  }
  return imp;
}

// Route every (tree, row) of positive weight from level l-1 to level l, and
// accumulate the class counts of every live node and the (slot, class, bin)
// histograms of the open ones.  A label byte >= C counts as class C - 1 (the
// caller validates labels; the device only keeps them inside the histogram).
__global__ __launch_bounds__(256) void rf_hist_multi_kernel(RfArgs A, int C, int level, int rows_per_block,
                                                            bool lds_hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = blockIdx.y;
  const int nodes = 1 << level;
  const int first = nodes - 1;
  const int n_inner = (1 << A.max_depth) - 1;
  const int n_all = 2 * n_inner + 1;
  const int node_ints = A.m * C * A.hb;
  int* cls_s = reinterpret_cast<int*>(smem);
  int* hist_s = cls_s + C * nodes;
  const int hist_n = lds_hist ? nodes * node_ints : 0;
  for (int e = threadIdx.x; e < C * nodes + hist_n; e += blockDim.x) cls_s[e] = 0;
  __syncthreads();
  int32_t* ghist = A.hist + static_cast<int64_t>(t) * nodes * node_ints;
  const uint8_t* st = A.status + static_cast<int64_t>(t) * n_all;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_block;
  const int64_t r1 = min(A.n, r0 + rows_per_block);
  for (int64_t i = r0 + threadIdx.x; i < r1; i += blockDim.x) {
    const int w = A.weights[static_cast<int64_t>(t) * A.n + i];
    if (w <= 0) continue;
    const Routed R = route_row(A, t, i, level, n_inner);
    if (!R.live) continue;
    const int h = R.h;
    const int local = h - first;
    const int y = min(static_cast<int>(A.labels[i]), C - 1);
    atomicAdd(&cls_s[C * local + y], w);
    if (st[h] != kOpen) continue;
    const int32_t* sub = A.subsets + (static_cast<int64_t>(t) * n_inner + h) * A.m;
    for (int s = 0; s < A.m; ++s) {
      const int b = min(static_cast<int>(A.bins[i * A.d + sub[s]]), A.hb - 1);
      const int o = ((local * A.m + s) * C + y) * A.hb + b;
      if (lds_hist) atomicAdd(&hist_s[o], w);
      else atomicAdd(&ghist[o], w);
    }
  }
  __syncthreads();
  int32_t* gcls = A.tot + static_cast<int64_t>(t) * nodes * C;
  for (int e = threadIdx.x; e < C * nodes; e += blockDim.x)
    if (cls_s[e]) atomicAdd(&gcls[e], cls_s[e]);
  for (int e = threadIdx.x; e < hist_n; e += blockDim.x)
    if (hist_s[e]) atomicAdd(&ghist[e], hist_s[e]);
}

// The leaf's class -- the first index of the largest weighted count
// (indexOfLargestArrayElement) -- over the leaf's heap subtree.
__device__ __forceinline__ void fill_leaf_multi(const RfArgs& A, int C, int t, int h, int level, const int32_t* gc) {
  const LeafSpan L = leaf_span(A, t, h, level);
  int best = 0;
  for (int c = 1; c < C; ++c)
    if (gc[c] > gc[best]) best = c;
  uint8_t* out = A.out_leaf + L.first;
  for (int q = 0; q < L.count; ++q) out[q] = static_cast<uint8_t>(best);  // (the loop is this kernel's: leaf_span)
}

// calculateImpurityStats (MLlib 2.1) for split k of slot s: left counts from
// the prefix sums (col[c * hb]), right = parent - left.  -DBL_MAX marks an
// invalid split.
__device__ __forceinline__ double split_gain_multi(const int* col, int hb, const int32_t* gc, int C, int64_t tc,
                                                   double parent_imp, int min_instances, double min_gain,
                                                   double* li_out, double* ri_out) {
  int64_t lc = 0;
  for (int c = 0; c < C; ++c) lc += col[c * hb];
  const int64_t rc = tc - lc;
  if (lc < min_instances || rc < min_instances) return -DBL_MAX;
  const double li = gini_c([&](int c) { return static_cast<int64_t>(col[c * hb]); }, C, lc);
  const double ri = gini_c([&](int c) { return static_cast<int64_t>(gc[c]) - col[c * hb]; }, C, rc);
  const double lw = static_cast<double>(lc) / static_cast<double>(tc);
  const double rw = static_cast<double>(rc) / static_cast<double>(tc);
  const double gain = parent_imp - lw * li - rw * ri;
  if (gain < min_gain) return -DBL_MAX;
  *li_out = li;
  *ri_out = ri;
  return gain;
}

// One block per node of the level: leaf class or best split.
__global__ __launch_bounds__(kSplitThreads) void rf_split_multi_kernel(RfArgs A, int C, unsigned char* red,
                                                                       int level) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* cum = reinterpret_cast<int*>(smem);  // [m][C][hb] prefix sums over bins
  const int t = blockIdx.y, local = blockIdx.x;
  const int nodes = 1 << level, h = nodes - 1 + local;
  const int n_inner = (1 << A.max_depth) - 1;
  const int n_all = 2 * n_inner + 1;
  uint8_t* st = A.status + static_cast<int64_t>(t) * n_all;
  const uint8_t s_h = st[h];  // (block-uniform: every return below is taken by the whole block)
  if (s_h == kAbsent) return;
  const int tid = threadIdx.x;
  const int32_t* gc = A.tot + (static_cast<int64_t>(t) * nodes + local) * C;
  if (s_h == kLeaf || level == A.max_depth) {
    if (tid == 0) {
      fill_leaf_multi(A, C, t, h, level, gc);
      if (h < n_inner) A.split_f[static_cast<int64_t>(t) * n_inner + h] = -1;
    }
    return;
  }
  const int node_ints = A.m * C * A.hb;
  const int32_t* gh = A.hist + (static_cast<int64_t>(t) * nodes + local) * node_ints;
  const int32_t* sub = A.subsets + (static_cast<int64_t>(t) * n_inner + h) * A.m;
  for (int e = tid; e < node_ints; e += kSplitThreads) cum[e] = gh[e];
  __syncthreads();
  prefix_sum_series(A, cum, C, sub, tid);
  __syncthreads();
  int64_t tc = 0;
  for (int c = 0; c < C; ++c) tc += gc[c];
  const double parent_imp = gini_c([&](int c) { return static_cast<int64_t>(gc[c]); }, C, tc);
  double best = -DBL_MAX;
  int best_p = INT_MAX;
  const int pairs = A.m * A.kmax;
  for (int p = tid; p < pairs; p += kSplitThreads) {
    const int s = p / A.kmax, k = p - s * A.kmax;
    if (k >= A.n_splits[sub[s]]) continue;
    double li, ri;
    const double g = split_gain_multi(cum + s * C * A.hb + k, A.hb, gc, C, tc, parent_imp, A.min_instances,
                                      A.min_gain, &li, &ri);
    if (g > best) {  // strict: a thread visits p in increasing order
      best = g;
      best_p = p;
    }
  }
  wave_first_max(best, best_p);
  block_first_max(red + (static_cast<int64_t>(t) * nodes + local) * kRedBytes, best, best_p, tid);
  if (tid != 0) return;
  if (!(best > 0.0)) {  // gain <= 0 or no valid split: leaf
    fill_leaf_multi(A, C, t, h, level, gc);
    A.split_f[static_cast<int64_t>(t) * n_inner + h] = -1;
    return;
  }
  const int s = best_p / A.kmax, k = best_p - s * A.kmax;
  double li = 0.0, ri = 0.0;
  split_gain_multi(cum + s * C * A.hb + k, A.hb, gc, C, tc, parent_imp, A.min_instances, A.min_gain, &li, &ri);
  commit_split(A, st, t, h, level, n_inner, sub[s], k, li, ri);
}

template <int32_t KIND>
struct ClassTrainer {
  using Job = RfJob;
  static constexpr int32_t kKind = KIND;

  // (n_classes sits before the outputs in the entries' argument lists)
  static int begin(RfJob* J, void* job, int64_t min_n, hipStream_t st, const float* x, int64_t n, int64_t d,
                   int64_t ldx, const uint8_t* labels, const float* thresholds, const int32_t* n_splits,
                   int32_t num_splits, const int32_t* weights, const int32_t* feature_subsets, int32_t m,
                   int32_t n_trees, int32_t max_depth, int32_t min_instances, double min_info_gain,
                   int32_t n_classes, int32_t* out_inner, uint8_t* out_leaf, void* ws, size_t ws_bytes) {
    return rf_classifier_begin(J, job, kKind, n_classes, min_n, st, x, n, d, ldx, labels, thresholds,
                               n_splits, num_splits, weights, feature_subsets, m, n_trees, max_depth, min_instances,
                               min_info_gain, out_inner, out_leaf, ws, ws_bytes);
  }

  // Zero the level's totals and histogram, then add the job's rows to them.
  static int level_stats(const RfJob& J, int level, hipStream_t st) {
    int64_t ints = 0;
    const RfArgs A = rf_at_level(J, level, &ints);
    const int C = J.C;
    if (hipMemsetAsync(A.tot, 0, static_cast<size_t>(ints) * 4, st) != hipSuccess) return DAL_ERR_HIP;
    if (A.n == 0) return DAL_OK;
    const int64_t nodes = int64_t{1} << level;
    const int64_t hist_ints = level < A.max_depth ? nodes * A.m * A.hb * C : 0;
    const int rows_per_block = 1024;
    const dim3 hgrid(static_cast<unsigned>(ceil_div(A.n, rows_per_block)), static_cast<unsigned>(A.T));
    // class counts + level histogram within the LDS budget, else global atomics
    const bool lds_hist = (C * nodes + hist_ints) * 4 <= kHistLdsBytes;
    const size_t hsmem = static_cast<size_t>(C * nodes + (lds_hist ? hist_ints : 0)) * 4;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(rf_hist_multi_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(hsmem)) != hipSuccess)
      return DAL_ERR_HIP;
    hipLaunchKernelGGL(rf_hist_multi_kernel, hgrid, dim3(256), hsmem, st, A, C, level, rows_per_block, lds_hist);
    DAL_RETURN_IF_LAUNCH_FAILED();
    return DAL_OK;
  }

  // Leaf or best split of every node of the level from the workspace's sums.
  static int level_split(const RfJob& J, int level, hipStream_t st) {
    int64_t ints = 0;
    const RfArgs A = rf_at_level(J, level, &ints);
    const size_t ssmem = level < A.max_depth ? static_cast<size_t>(A.m) * A.hb * J.C * 4 : 16;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(rf_split_multi_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(ssmem)) != hipSuccess)
      return DAL_ERR_HIP;
    hipLaunchKernelGGL(rf_split_multi_kernel, dim3(1u << level, static_cast<unsigned>(A.T)), dim3(kSplitThreads),
                       ssmem, st, A, J.C, J.red, level);
    DAL_RETURN_IF_LAUNCH_FAILED();
    return DAL_OK;
  }

  static int finish(const RfJob& J, hipStream_t st) { return rf_launch_finalize(J.A, st); }
};
using Multi = RfLadder<ClassTrainer<kRfJobMulti>>;

// The binary entries: two classes, and no n_classes in their argument lists.
struct BinaryTrainer : ClassTrainer<kRfJobBinary> {
  template <class... Args>
  static int begin(RfJob* J, void* job, int64_t min_n, hipStream_t st, Args... args) {
    return rf_classifier_begin(J, job, kKind, 2, min_n, st, args...);
  }
};
using Binary = RfLadder<BinaryTrainer>;

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" size_t dal_rf_train_multiclass_workspace_bytes(int64_t n, int64_t d, int32_t n_trees, int32_t max_depth,
                                                          int32_t m, int32_t num_splits, int32_t n_classes) {
  if (n < 1 || d < 1 || n_trees < 1 || max_depth < 1 || max_depth > DAL_RF_MAX_DEPTH || m < 1 || num_splits < 0 ||
      n_classes < 2 || n_classes > DAL_MC_MAX_CLASSES)
    return 0;
  return rf_layout(n * d, n, n_trees, max_depth, m, num_splits + 2, n_classes, 4, kRedBytes).total;
}

extern "C" int dal_rf_train_multiclass_begin(void* job, const float* x, int64_t n_local, int64_t d, int64_t ldx,
                                             const uint8_t* labels, const float* thresholds,
                                             const int32_t* n_splits, int32_t num_splits, const int32_t* weights,
                                             const int32_t* feature_subsets, int32_t m, int32_t n_trees,
                                             int32_t max_depth, int32_t min_instances, double min_info_gain,
                                             int32_t n_classes, int32_t* out_inner, uint8_t* out_leaf, void* ws,
                                             size_t ws_bytes, dal_stream_t stream) {
  return Multi::begin(job, stream, x, n_local, d, ldx, labels, thresholds, n_splits, num_splits, weights,
                      feature_subsets, m, n_trees, max_depth, min_instances, min_info_gain, n_classes, out_inner,
                      out_leaf, ws, ws_bytes);
}

extern "C" int dal_rf_train_multiclass_level_stats(const void* job, int32_t level, dal_stream_t stream) {
  return Multi::level_stats(job, level, stream);
}

extern "C" int dal_rf_train_multiclass_level_split(const void* job, int32_t level, dal_stream_t stream) {
  return Multi::level_split(job, level, stream);
}

extern "C" int dal_rf_train_multiclass_finish(const void* job, dal_stream_t stream) {
  return Multi::finish(job, stream);
}

extern "C" int dal_rf_train_multiclass_level_span(const void* job, int32_t level, void** ptr, int32_t* elem_type,
                                                  int64_t* count) {
  return Multi::level_span(job, level, ptr, elem_type, count);
}

extern "C" int dal_rf_train_multiclass(const float* x, int64_t n, int64_t d, int64_t ldx, const uint8_t* labels,
                                       const float* thresholds, const int32_t* n_splits, int32_t num_splits,
                                       const int32_t* weights, const int32_t* feature_subsets, int32_t m,
                                       int32_t n_trees, int32_t max_depth, int32_t min_instances,
                                       double min_info_gain, int32_t n_classes, int32_t* out_inner,
                                       uint8_t* out_leaf, void* ws, size_t ws_bytes, dal_stream_t stream) {
  return Multi::fit(stream, x, n, d, ldx, labels, thresholds, n_splits, num_splits, weights, feature_subsets, m,
                    n_trees, max_depth, min_instances, min_info_gain, n_classes, out_inner, out_leaf, ws, ws_bytes);
}

extern "C" size_t dal_rf_train_workspace_bytes(int64_t n, int64_t d, int32_t n_trees, int32_t max_depth, int32_t m,
                                               int32_t num_splits) {
  return dal_rf_train_multiclass_workspace_bytes(n, d, n_trees, max_depth, m, num_splits, 2);
}

extern "C" int dal_rf_train_begin(void* job, const float* x, int64_t n_local, int64_t d, int64_t ldx,
                                  const uint8_t* labels, const float* thresholds, const int32_t* n_splits,
                                  int32_t num_splits, const int32_t* weights, const int32_t* feature_subsets,
                                  int32_t m, int32_t n_trees, int32_t max_depth, int32_t min_instances,
                                  double min_info_gain, int32_t* out_inner, uint8_t* out_leaf, void* ws,
                                  size_t ws_bytes, dal_stream_t stream) {
  return Binary::begin(job, stream, x, n_local, d, ldx, labels, thresholds, n_splits, num_splits, weights,
                       feature_subsets, m, n_trees, max_depth, min_instances, min_info_gain, out_inner, out_leaf, ws,
                       ws_bytes);
}

extern "C" int dal_rf_train_level_stats(const void* job, int32_t level, dal_stream_t stream) {
  return Binary::level_stats(job, level, stream);
}

extern "C" int dal_rf_train_level_split(const void* job, int32_t level, dal_stream_t stream) {
  return Binary::level_split(job, level, stream);
}

extern "C" int dal_rf_train_finish(const void* job, dal_stream_t stream) { return Binary::finish(job, stream); }

extern "C" int dal_rf_train_level_span(const void* job, int32_t level, void** ptr, int32_t* elem_type,
                                       int64_t* count) {
  return Binary::level_span(job, level, ptr, elem_type, count);
}

extern "C" int dal_rf_train(const float* x, int64_t n, int64_t d, int64_t ldx, const uint8_t* labels,
                            const float* thresholds, const int32_t* n_splits, int32_t num_splits,
                            const int32_t* weights, const int32_t* feature_subsets, int32_t m, int32_t n_trees,
                            int32_t max_depth, int32_t min_instances, double min_info_gain, int32_t* out_inner,
                            uint8_t* out_leaf, void* ws, size_t ws_bytes, dal_stream_t stream) {
  return Binary::fit(stream, x, n, d, ldx, labels, thresholds, n_splits, num_splits, weights, feature_subsets, m,
                     n_trees, max_depth, min_instances, min_info_gain, out_inner, out_leaf, ws, ws_bytes);
}
