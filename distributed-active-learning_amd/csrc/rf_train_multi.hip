// Random-forest training on the GPU for C classes (2 <= C <= DAL_MC_MAX_CLASSES):
//   RandomForest.trainClassifier(train, numClasses=C, categoricalFeaturesInfo={},
//                                numTrees=T, featureSubsetStrategy="auto",
//                                impurity='gini', maxDepth=4, maxBins=32)
//   final_thesis/uncertainty_sampling.py:71-76, density_weighting.py:119-124
// The algorithm is the one of rf_train.hip (its header comment has the steps)
// with C classes wherever two appear there; thresholds, binning, the status
// reset and the heap finalize do not depend on the labels and are that file's
// (rf_train_shared.hpp).  The binary kernels stay as they are: this file adds
// the two level kernels for a class axis.
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
#include <algorithm>
#include <cfloat>
#include <climits>

#include "common.hpp"
#include "rf_train_shared.hpp"

namespace dal {
namespace {

constexpr int kSplitThreads = 256;
constexpr int kSplitWaves = kSplitThreads / kWave;
constexpr int kRedBytes = 64;  // per node: kSplitWaves gains (fp64) then kSplitWaves pair indices (int32)

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
    int32_t* nd = A.node + static_cast<int64_t>(t) * A.n + i;
    int h = 0;
    if (level > 0) {
      const int hp = *nd;
      if (hp < 0) continue;
      const int f = A.split_f[static_cast<int64_t>(t) * n_inner + hp];
      if (f < 0) {  // the row's node became a leaf
        *nd = -1;
        continue;
      }
      const int b = A.bins[i * A.d + f];
      h = 2 * hp + 1 + (b > A.split_b[static_cast<int64_t>(t) * n_inner + hp] ? 1 : 0);
    }
    *nd = h;
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
  int32_t* gcls = A.cls + static_cast<int64_t>(t) * nodes * C;
  for (int e = threadIdx.x; e < C * nodes; e += blockDim.x)
    if (cls_s[e]) atomicAdd(&gcls[e], cls_s[e]);
  for (int e = threadIdx.x; e < hist_n; e += blockDim.x)
    if (hist_s[e]) atomicAdd(&ghist[e], hist_s[e]);
}

// The leaf's class -- the first index of the largest weighted count
// (indexOfLargestArrayElement) -- over the leaf's heap subtree.
__device__ __forceinline__ void fill_leaf_multi(const RfArgs& A, int C, int t, int h, int level, const int32_t* gc) {
  const int n_inner = (1 << A.max_depth) - 1;
  const int span = 1 << (A.max_depth - level);
  const int first_leaf = (h + 1) * span - 1 - n_inner;
  int best = 0;
  for (int c = 1; c < C; ++c)
    if (gc[c] > gc[best]) best = c;
  uint8_t* out = A.out_leaf + static_cast<int64_t>(t) * (n_inner + 1) + first_leaf;
  for (int q = 0; q < span; ++q) out[q] = static_cast<uint8_t>(best);
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
  const int32_t* gc = A.cls + (static_cast<int64_t>(t) * nodes + local) * C;
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
  for (int q = tid; q < A.m * C; q += kSplitThreads) {
    const int nb = min(A.n_splits[sub[q / C]] + 1, A.hb);
    int* row = cum + q * A.hb;
    int a = 0;
    for (int b = 0; b < nb; ++b) {
      a += row[b];
      row[b] = a;
    }
  }
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
  // lexicographic first maximum over (gain desc, pair index asc): the wave, then the block
  for (int o = 32; o > 0; o >>= 1) {
    const double og = __shfl_xor(best, o);
    const int op = __shfl_xor(best_p, o);
    if (og > best || (og == best && op < best_p)) {
      best = og;
      best_p = op;
    }
  }
  unsigned char* r = red + (static_cast<int64_t>(t) * nodes + local) * kRedBytes;
  double* red_g = reinterpret_cast<double*>(r);
  int* red_p = reinterpret_cast<int*>(r + kSplitWaves * 8);
  if ((tid & (kWave - 1)) == 0) {
    red_g[tid / kWave] = best;
    red_p[tid / kWave] = best_p;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores have left this wave before the barrier
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < kSplitWaves; ++w) {
    const double og = red_g[w];
    const int op = red_p[w];
    if (og > best || (og == best && op < best_p)) {
      best = og;
      best_p = op;
    }
  }
  if (!(best > 0.0)) {  // gain <= 0 or no valid split: leaf
    fill_leaf_multi(A, C, t, h, level, gc);
    A.split_f[static_cast<int64_t>(t) * n_inner + h] = -1;
    return;
  }
  const int s = best_p / A.kmax, k = best_p - s * A.kmax;
  double li = 0.0, ri = 0.0;
  split_gain_multi(cum + s * C * A.hb + k, A.hb, gc, C, tc, parent_imp, A.min_instances, A.min_gain, &li, &ri);
  A.split_f[static_cast<int64_t>(t) * n_inner + h] = sub[s];
  A.split_b[static_cast<int64_t>(t) * n_inner + h] = k;
  const bool child_leaf = level + 1 == A.max_depth;
  st[2 * h + 1] = (child_leaf || li == 0.0) ? kLeaf : kOpen;
  st[2 * h + 2] = (child_leaf || ri == 0.0) ? kLeaf : kOpen;
}

bool multi_shape_ok(int64_t n, int64_t d, int32_t n_trees, int32_t max_depth, int32_t m, int32_t num_splits,
                    int32_t n_classes) {
  return n >= 1 && d >= 1 && n_trees >= 1 && max_depth >= 1 && max_depth <= DAL_RF_MAX_DEPTH && m >= 1 &&
         num_splits >= 0 && n_classes >= 2 && n_classes <= DAL_MC_MAX_CLASSES;
}

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" size_t dal_rf_train_multiclass_workspace_bytes(int64_t n, int64_t d, int32_t n_trees, int32_t max_depth,
                                                          int32_t m, int32_t num_splits, int32_t n_classes) {
  if (!multi_shape_ok(n, d, n_trees, max_depth, m, num_splits, n_classes)) return 0;
  return rf_layout(n, d, n_trees, max_depth, m, num_splits + 2, n_classes, kRedBytes).total;
}

namespace dal {
namespace {

// *J is the job; it is also copied to the caller's descriptor `job` (nullable)
// before the first device call.
int multi_begin(RfJob* J, void* job, const float* x, int64_t n, int64_t d, int64_t ldx, const uint8_t* labels,
                const float* thresholds, const int32_t* n_splits, int32_t num_splits, const int32_t* weights,
                const int32_t* feature_subsets, int32_t m, int32_t n_trees, int32_t max_depth, int32_t min_instances,
                double min_info_gain, int32_t n_classes, int32_t* out_inner, uint8_t* out_leaf, void* ws,
                size_t ws_bytes, int64_t min_n, hipStream_t st) {
  if (const int rc = rf_job_setup(J, kRfJobMulti, n_classes, kRedBytes, x, n, d, ldx, labels, thresholds, n_splits,
                                  num_splits, weights, feature_subsets, m, n_trees, max_depth, min_instances,
                                  min_info_gain, out_inner, out_leaf, ws, ws_bytes, min_n))
    return rc;
  if (job) std::memcpy(job, J, sizeof *J);
  return rf_launch_bin_and_reset(x, ldx, J->A, st);
}

// Zero the level's totals and histogram, then add the job's rows to them.
int multi_level_stats(const RfJob& J, int level, hipStream_t st) {
  int64_t ints = 0;
  const RfArgs A = rf_at_level(J, level, &ints);
  const int C = J.C;
  if (hipMemsetAsync(A.cls, 0, static_cast<size_t>(ints) * 4, st) != hipSuccess) return DAL_ERR_HIP;
  if (A.n == 0) return DAL_OK;
  const int64_t nodes = int64_t{1} << level;
  const int64_t hist_ints = level < A.max_depth ? nodes * A.m * A.hb * C : 0;
  const int rows_per_block = 1024;
  const dim3 hgrid(static_cast<unsigned>(ceil_div(A.n, rows_per_block)), static_cast<unsigned>(A.T));
  // the budget of the binary kernel: class counts + level histogram within 64 KiB, else global atomics
  const bool lds_hist = (C * nodes + hist_ints) * 4 <= 64 * 1024;
  const size_t hsmem = static_cast<size_t>(C * nodes + (lds_hist ? hist_ints : 0)) * 4;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(rf_hist_multi_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(hsmem)) != hipSuccess)
    return DAL_ERR_HIP;
  hipLaunchKernelGGL(rf_hist_multi_kernel, hgrid, dim3(256), hsmem, st, A, C, level, rows_per_block, lds_hist);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

// Leaf or best split of every node of the level from the workspace's sums.
int multi_level_split(const RfJob& J, int level, hipStream_t st) {
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

}  // namespace
}  // namespace dal

extern "C" int dal_rf_train_multiclass_begin(void* job, const float* x, int64_t n_local, int64_t d, int64_t ldx,
                                             const uint8_t* labels, const float* thresholds,
                                             const int32_t* n_splits, int32_t num_splits, const int32_t* weights,
                                             const int32_t* feature_subsets, int32_t m, int32_t n_trees,
                                             int32_t max_depth, int32_t min_instances, double min_info_gain,
                                             int32_t n_classes, int32_t* out_inner, uint8_t* out_leaf, void* ws,
                                             size_t ws_bytes, dal_stream_t stream) {
  RfJob J;
  if (!job) return DAL_ERR_ARG;
  return multi_begin(&J, job, x, n_local, d, ldx, labels, thresholds, n_splits, num_splits, weights, feature_subsets, m,
                     n_trees, max_depth, min_instances, min_info_gain, n_classes, out_inner, out_leaf, ws, ws_bytes,
                     0, as_stream(stream));
}

extern "C" int dal_rf_train_multiclass_level_stats(const void* job, int32_t level, dal_stream_t stream) {
  RfJob J;
  if (const int rc = rf_job_load(job, kRfJobMulti, level, &J)) return rc;
  return multi_level_stats(J, level, as_stream(stream));
}

extern "C" int dal_rf_train_multiclass_level_split(const void* job, int32_t level, dal_stream_t stream) {
  RfJob J;
  if (const int rc = rf_job_load(job, kRfJobMulti, level, &J)) return rc;
  return multi_level_split(J, level, as_stream(stream));
}

extern "C" int dal_rf_train_multiclass_finish(const void* job, dal_stream_t stream) {
  RfJob J;
  if (const int rc = rf_job_load(job, kRfJobMulti, 0, &J)) return rc;
  return rf_launch_finalize(J.A, as_stream(stream));
}

extern "C" int dal_rf_train_multiclass_level_span(const void* job, int32_t level, void** ptr, int32_t* elem_type,
                                                  int64_t* count) {
  return rf_level_span(job, kRfJobMulti, level, ptr, elem_type, count);
}

extern "C" int dal_rf_train_multiclass(const float* x, int64_t n, int64_t d, int64_t ldx, const uint8_t* labels,
                                       const float* thresholds, const int32_t* n_splits, int32_t num_splits,
                                       const int32_t* weights, const int32_t* feature_subsets, int32_t m,
                                       int32_t n_trees, int32_t max_depth, int32_t min_instances,
                                       double min_info_gain, int32_t n_classes, int32_t* out_inner,
                                       uint8_t* out_leaf, void* ws, size_t ws_bytes, dal_stream_t stream) {
  RfJob J;
  hipStream_t st = as_stream(stream);
  if (const int rc = multi_begin(&J, nullptr, x, n, d, ldx, labels, thresholds, n_splits, num_splits, weights,
                                 feature_subsets, m, n_trees, max_depth, min_instances, min_info_gain, n_classes,
                                 out_inner, out_leaf, ws, ws_bytes, 1, st))
    return rc;
  for (int level = 0; level <= max_depth; ++level) {
    if (const int rc = multi_level_stats(J, level, st)) return rc;
    if (const int rc = multi_level_split(J, level, st)) return rc;
  }
  return rf_launch_finalize(J.A, st);
}
