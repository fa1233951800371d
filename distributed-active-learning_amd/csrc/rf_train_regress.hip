// Regression-forest training on the GPU:
//   RandomForest.trainRegressor(data, categoricalFeaturesInfo={}, numTrees=T,
//                               featureSubsetStrategy="auto", impurity="variance",
//                               maxDepth=4, maxBins=32)
//   lal_direct_mllib_implementation/classes/active_learner.py:354-365 (the LAL
//   model, 2,000 trees), mllib/mllib_randomforest_regression_lal_randomtree_dataset.py:30
// Spark 2.1 MLlib, continuous features.  Thresholds, bins, bagging weights,
// feature subsets, level-wise growth, the first-maximum rule and the leaf
// rules are those of rf_train.hip / rf_train_multi.hip (their header comments
// have the steps); the impurity is MLlib's Variance over (count, sum, sumSq).
//
// Gini histograms are integer sums.  Variance needs sum w*y and sum w*fl(y*y)
// per (node, slot, bin), and an fp64 atomicAdd would make them -- and with
// them leaves and, under cancellation, the chosen splits -- depend on the
// arrival order.  Here every cell is an exact integer accumulator
// (rf_exact_sum.hpp): (count, K_y limbs of y, K_sq limbs of y*y) int64 words,
// added with 64-bit integer atomics, so a histogram is exact in any order and
// a fit is reproducible bit for bit.  Each statistic is rounded to fp64 once.
//
//   histogram  [tree][node][slot][word][bin], bins innermost (the split
//              kernel's lanes take consecutive split indices);  LDS while the
//              level's totals + histogram fit 64 KiB (the classifiers'
//              budget), flushed once per block; else global atomics.
//   split      one block of 4 waves per node: the node's cells go to LDS,
//              every (slot, word) series is prefix-summed over bins (exact),
//              left = prefix, right = node total - left word by word (exact),
//              each of the four sums is rounded once, then
//              Variance.calculate and the gain in fp64 in MLlib's order, no
//              FMA; the lexicographic first maximum as rf_split_multi_kernel.
//
// This file owns the two level kernels over exact cells, the variance and the
// fp64 finalize; the threshold search and binning (its fp64 forms are
// instantiated here), routing, prefix sums, the first-maximum reduction, the
// commit and the entry ladder are rf_train_device.hpp's, the workspace
// layout, the level view and the status reset rf_train_shared.hpp's.
#include "common.hpp"
#include "rf_exact_sum.hpp"
#include "rf_train_device.hpp"

namespace dal {
namespace {

struct RegArgs {
  const uint8_t* bins;       // [n][d]
  const double* y;           // [n]
  const int32_t* weights;    // [T][n]
  const int32_t* subsets;    // [T][n_inner][m]
  const double* thresholds;  // [d][DAL_RF_MAX_SPLITS]
  const int32_t* n_splits;   // [d]
  int64_t n;
  int d, m, T, max_depth, hb, kmax;
  int min_instances;
  double min_gain;
  int q_y, k_y, q_sq, k_sq, W;  // W = 1 + k_y + k_sq words per cell: count, limbs of y, limbs of fl(y*y)
  int32_t* node;      // [T][n] heap index at the previous level (-1 settled)
  uint8_t* status;    // [T][n_all]
  int32_t* split_f;   // [T][n_inner]
  int32_t* split_b;   // [T][n_inner]
  int64_t* hist;      // [T][2^l][m][W][hb], the current level
  int64_t* tot;       // [T][2^l][W], ending where hist begins (rf_at_level)
  int32_t* out_feature;   // [T][n_inner]
  double* out_threshold;  // [T][n_inner]
  double* out_leaf;       // [T][n_leaf]
};

// The job descriptor of the level steps (rf_train_shared.hpp has the
// classifiers'); A.tot holds the END of the totals piece (== A.hist).
struct RegJob {
  uint32_t magic;
  int32_t kind;
  unsigned char* red;
  RegArgs A;
  int64_t words() const { return A.W; }  // per cell
};
static_assert(sizeof(RegJob) <= DAL_RF_JOB_BYTES, "DAL_RF_JOB_BYTES holds a regressor job");

// The caller's binned rows: no bins piece.
RfLayout reg_layout(int64_t n, int64_t T, int max_depth, int64_t m, int64_t hb, int64_t W) {
  return rf_layout(0, n, T, max_depth, m, hb, W, 8, kRedBytes);
}

// Two's complement adds: a signed word through the unsigned 64-bit atomic.
__device__ __forceinline__ void add64(int64_t* p, int64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(v));
}

// Route every (tree, row) of positive weight from level l-1 to level l, and
// add its (w, w * limbs of y, w * limbs of y*y) to the totals of its node and
// to the (slot, bin) cells of an open node.  A zero limb adds nothing.
__global__ __launch_bounds__(256) void rf_hist_regress_kernel(RegArgs A, int level, int rows_per_block,
                                                              bool lds_tot, bool lds_hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = blockIdx.y;
  const int nodes = 1 << level;
  const int first = nodes - 1;
  const int n_inner = (1 << A.max_depth) - 1;
  const int n_all = 2 * n_inner + 1;
  const int W = A.W, hb = A.hb;
  const int node_words = A.m * W * hb;
  const int tot_n = lds_tot ? nodes * W : 0;
  const int hist_n = lds_hist ? nodes * node_words : 0;
  int64_t* tot_s = reinterpret_cast<int64_t*>(smem);
  int64_t* hist_s = tot_s + tot_n;
  for (int e = threadIdx.x; e < tot_n + hist_n; e += blockDim.x) tot_s[e] = 0;
  __syncthreads();
  int64_t* gtot = A.tot + static_cast<int64_t>(t) * nodes * W;
  int64_t* ghist = A.hist + static_cast<int64_t>(t) * nodes * node_words;
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
    const double y = A.y[i];
    const exact::Parts py = exact::parts(y), pq = exact::parts(y * y);
    int64_t ly[exact::kMaxLimbs], lq[exact::kMaxLimbs];  // w * limb; fixed indices: registers
#pragma unroll
    for (int j = 0; j < exact::kMaxLimbs; ++j) {
      ly[j] = j < A.k_y ? static_cast<int64_t>(w) * exact::limb(py, A.q_y, j) : 0;
      lq[j] = j < A.k_sq ? static_cast<int64_t>(w) * exact::limb(pq, A.q_sq, j) : 0;
    }
    // one cell: word k at p[k * stride]
    auto add_cell = [&](int64_t* p, int stride) {
      add64(p, w);
#pragma unroll
      for (int j = 0; j < exact::kMaxLimbs; ++j)
        if (ly[j]) add64(p + (1 + j) * stride, ly[j]);
#pragma unroll
      for (int j = 0; j < exact::kMaxLimbs; ++j)
        if (lq[j]) add64(p + (1 + A.k_y + j) * stride, lq[j]);
    };
    if (lds_tot) add_cell(tot_s + local * W, 1);
    else add_cell(gtot + local * W, 1);
    if (st[h] != kOpen) continue;
    const int32_t* sub = A.subsets + (static_cast<int64_t>(t) * n_inner + h) * A.m;
    for (int s = 0; s < A.m; ++s) {
      const int b = min(static_cast<int>(A.bins[i * A.d + sub[s]]), hb - 1);
      const int o = (local * A.m + s) * W * hb + b;
      if (lds_hist) add_cell(hist_s + o, hb);
      else add_cell(ghist + o, hb);
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < tot_n; e += blockDim.x)
    if (tot_s[e]) add64(&gtot[e], tot_s[e]);
  for (int e = threadIdx.x; e < hist_n; e += blockDim.x)
    if (hist_s[e]) add64(&ghist[e], hist_s[e]);
}

// Variance.calculate: 0 when count == 0, else (sumSq - (sum * sum) / count) / count.
__device__ __forceinline__ double variance(int64_t count, double sum, double sum_sq) {
  if (count == 0) return 0.0;
  const double c = static_cast<double>(count);
  return (sum_sq - (sum * sum) / c) / c;
}

// The leaf's value, sum / count (0 for no rows), over the leaf's heap subtree.
__device__ __forceinline__ void fill_leaf_regress(const RegArgs& A, int t, int h, int level, const int64_t* gt) {
  const LeafSpan L = leaf_span(A, t, h, level);
  const int64_t count = gt[0];
  double v = 0.0;
  if (count != 0) v = exact::to_double([&](int j) { return gt[1 + j]; }, A.k_y, A.q_y) / static_cast<double>(count);
  double* out = A.out_leaf + L.first;
  for (int q = 0; q < L.count; ++q) out[q] = v;  // (the loop is this kernel's: leaf_span)
}

// calculateImpurityStats (MLlib 2.1) for split k of slot s: the left cell is
// the prefix sum (col[word * hb]), the right cell the node's minus it, word by
// word; each sum is rounded once.  -DBL_MAX marks an invalid split.
__device__ __forceinline__ double split_gain_regress(const RegArgs& A, const int64_t* col, const int64_t* gt,
                                                     int64_t tc, double parent_imp, double* li_out,
                                                     double* ri_out) {
  const int hb = A.hb, ky = A.k_y;
  const int64_t lc = col[0];
  const int64_t rc = tc - lc;
  if (lc < A.min_instances || rc < A.min_instances) return -DBL_MAX;
  const double ls = exact::to_double([&](int j) { return col[(1 + j) * hb]; }, ky, A.q_y);
  const double lq = exact::to_double([&](int j) { return col[(1 + ky + j) * hb]; }, A.k_sq, A.q_sq);
  const double rs = exact::to_double([&](int j) { return gt[1 + j] - col[(1 + j) * hb]; }, ky, A.q_y);
  const double rq =
      exact::to_double([&](int j) { return gt[1 + ky + j] - col[(1 + ky + j) * hb]; }, A.k_sq, A.q_sq);
  const double li = variance(lc, ls, lq), ri = variance(rc, rs, rq);
  const double lw = static_cast<double>(lc) / static_cast<double>(tc);
  const double rw = static_cast<double>(rc) / static_cast<double>(tc);
  const double gain = parent_imp - lw * li - rw * ri;
  if (gain < A.min_gain) return -DBL_MAX;
  *li_out = li;
  *ri_out = ri;
  return gain;
}

// One block per node of the level: leaf value or best split.
__global__ __launch_bounds__(kSplitThreads) void rf_split_regress_kernel(RegArgs A, unsigned char* red, int level) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int64_t* cum = reinterpret_cast<int64_t*>(smem);  // [m][W][hb] prefix sums over bins
  const int t = blockIdx.y, local = blockIdx.x;
  const int nodes = 1 << level, h = nodes - 1 + local;
  const int n_inner = (1 << A.max_depth) - 1;
  const int n_all = 2 * n_inner + 1;
  uint8_t* st = A.status + static_cast<int64_t>(t) * n_all;
  const uint8_t s_h = st[h];  // (block-uniform: every return below is taken by the whole block)
  if (s_h == kAbsent) return;
  const int tid = threadIdx.x;
  const int W = A.W, hb = A.hb;
  const int64_t* gt = A.tot + (static_cast<int64_t>(t) * nodes + local) * W;
  if (s_h == kLeaf || level == A.max_depth) {
    if (tid == 0) {
      fill_leaf_regress(A, t, h, level, gt);
      if (h < n_inner) A.split_f[static_cast<int64_t>(t) * n_inner + h] = -1;
    }
    return;
  }
  const int node_words = A.m * W * hb;
  const int64_t* gh = A.hist + (static_cast<int64_t>(t) * nodes + local) * node_words;
  const int32_t* sub = A.subsets + (static_cast<int64_t>(t) * n_inner + h) * A.m;
  for (int e = tid; e < node_words; e += kSplitThreads) cum[e] = gh[e];
  __syncthreads();
  prefix_sum_series(A, cum, W, sub, tid);
  __syncthreads();
  const int64_t tc = gt[0];
  const double parent_imp =
      variance(tc, exact::to_double([&](int j) { return gt[1 + j]; }, A.k_y, A.q_y),
               exact::to_double([&](int j) { return gt[1 + A.k_y + j]; }, A.k_sq, A.q_sq));
  double best = -DBL_MAX;
  int best_p = INT_MAX;
  const int pairs = A.m * A.kmax;
  for (int p = tid; p < pairs; p += kSplitThreads) {
    const int s = p / A.kmax, k = p - s * A.kmax;
    if (k >= A.n_splits[sub[s]]) continue;
    double li, ri;
    const double g = split_gain_regress(A, cum + s * W * hb + k, gt, tc, parent_imp, &li, &ri);
    if (g > best) {  // strict: a thread visits p in increasing order
      best = g;
      best_p = p;
    }
  }
  wave_first_max(best, best_p);
  block_first_max(red + (static_cast<int64_t>(t) * nodes + local) * kRedBytes, best, best_p, tid);
  if (tid != 0) return;
  if (!(best > 0.0)) {  // gain <= 0 or no valid split: leaf
    fill_leaf_regress(A, t, h, level, gt);
    A.split_f[static_cast<int64_t>(t) * n_inner + h] = -1;
    return;
  }
  const int s = best_p / A.kmax, k = best_p - s * A.kmax;
  double li = 0.0, ri = 0.0;
  split_gain_regress(A, cum + s * W * hb + k, gt, tc, parent_imp, &li, &ri);
  commit_split(A, st, t, h, level, n_inner, sub[s], k, li, ri);
}

// RegressionForest's heap arrays: (feature, fp64 threshold) per inner node;
// absent / leaf positions become always-left (0, +inf) padding.
__global__ void rf_finalize_regress_kernel(RegArgs A) {
  const int n_inner = (1 << A.max_depth) - 1;
  const int64_t total = static_cast<int64_t>(A.T) * n_inner;
  for (int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; e < total;
       e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int t = static_cast<int>(e / n_inner), h = static_cast<int>(e - static_cast<int64_t>(t) * n_inner);
    const uint8_t s = A.status[static_cast<int64_t>(t) * (2 * n_inner + 1) + h];
    const int f = s == kAbsent ? -1 : A.split_f[e];
    A.out_feature[e] = f >= 0 ? f : 0;
    A.out_threshold[e] = f >= 0 ? A.thresholds[static_cast<int64_t>(f) * DAL_RF_MAX_SPLITS + A.split_b[e]]
                                : static_cast<double>(__builtin_inff());
  }
}

bool limbs_ok(int32_t q, int32_t k) { return k >= 1 && k <= DAL_RF_REG_MAX_LIMBS && q >= -1074 && q <= 1023; }

int64_t max_sample(int x_dtype) {
  return x_dtype == DAL_X_F64 ? DAL_RF_MAX_SPLIT_SAMPLE_F64 : DAL_RF_MAX_SPLIT_SAMPLE;
}

struct RegressTrainer {
  using Job = RegJob;
  static constexpr int32_t kKind = kRfJobRegress;

  // The argument checks of dal_rf_train_regressor over n >= min_n rows, the
  // workspace layout, the job, then the status reset.  bins, y and weights may
  // be null for a job of no rows.  *Jp is the job; it is also copied to the
  // caller's descriptor `job` (nullable) before the first device call.
  static int begin(RegJob* Jp, void* job, int64_t min_n, hipStream_t st, const uint8_t* bins, int64_t n, int64_t d,
                   const double* y, const double* thresholds, const int32_t* n_splits, int32_t num_splits,
                   const int32_t* weights, const int32_t* feature_subsets, int32_t m, int32_t n_trees,
                   int32_t max_depth, int32_t min_instances, double min_info_gain, int32_t q_y, int32_t k_y,
                   int32_t q_sq, int32_t k_sq, int32_t* out_feature, double* out_threshold, double* out_leaf,
                   void* ws, size_t ws_bytes) {
    if (!thresholds || !n_splits || !feature_subsets || !out_feature || !out_threshold || !out_leaf || !ws)
      return DAL_ERR_ARG;
    if ((n > 0 || min_n > 0) && (!bins || !y || !weights)) return DAL_ERR_ARG;
    if (n < min_n || d < 1 || n_trees < 1 || m < 1 || m > d) return DAL_ERR_SHAPE;
    if (max_depth < 1 || max_depth > DAL_RF_MAX_DEPTH) return DAL_ERR_UNSUPPORTED;
    if (!limbs_ok(q_y, k_y) || !limbs_ok(q_sq, k_sq)) return DAL_ERR_UNSUPPORTED;
    if (num_splits < 0 || num_splits >= DAL_RF_MAX_SPLITS) return DAL_ERR_SHAPE;
    const int hb = num_splits + 2;  // find_splits emits at most num_splits + 1 thresholds
    const int W = 1 + k_y + k_sq;
    // the split kernel keeps one node's whole (slot, word, bin) histogram in LDS
    if (static_cast<int64_t>(m) * hb * W * 8 > DAL_RF_SPLIT_LDS_BYTES) return DAL_ERR_UNSUPPORTED;
    const RfLayout L = reg_layout(n, n_trees, max_depth, m, hb, W);
    if (ws_bytes < L.total || reinterpret_cast<uintptr_t>(ws) % 256) return DAL_ERR_SHAPE;
    unsigned char* w = static_cast<unsigned char*>(ws);
    RegJob& J = *Jp;
    J = RegJob{};
    J.magic = kRfJobMagic;
    J.kind = kKind;
    J.red = w + L.red;
    RegArgs& A = J.A;
    A.bins = bins;
    A.y = y;
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
    A.q_y = q_y;
    A.k_y = k_y;
    A.q_sq = q_sq;
    A.k_sq = k_sq;
    A.W = W;
    A.node = reinterpret_cast<int32_t*>(w + L.node);
    A.status = w + L.status;
    A.split_f = reinterpret_cast<int32_t*>(w + L.split_f);
    A.split_b = reinterpret_cast<int32_t*>(w + L.split_b);
    A.hist = reinterpret_cast<int64_t*>(w + L.hist);
    A.tot = A.hist;
    A.out_feature = out_feature;
    A.out_threshold = out_threshold;
    A.out_leaf = out_leaf;
    if (job) std::memcpy(job, &J, sizeof J);
    return rf_launch_reset(A.status, n_trees, max_depth, st);
  }

  // Zero the level's totals and histogram, then add the job's rows to them.
  static int level_stats(const RegJob& J, int level, hipStream_t st) {
    int64_t words = 0;
    const RegArgs A = rf_at_level(J, level, &words);
    if (hipMemsetAsync(A.tot, 0, static_cast<size_t>(words) * 8, st) != hipSuccess) return DAL_ERR_HIP;
    if (A.n == 0) return DAL_OK;
    const int64_t nodes = int64_t{1} << level;
    const bool open_level = level < A.max_depth;
    const int64_t tot_bytes = nodes * A.W * 8;
    const int64_t hist_bytes = open_level ? nodes * A.m * A.hb * A.W * 8 : 0;
    const int rows_per_block = 1024;
    const dim3 hgrid(static_cast<unsigned>(ceil_div(A.n, rows_per_block)), static_cast<unsigned>(A.T));
    // totals + level histogram within the LDS budget, else global atomics
    const bool lds_tot = tot_bytes <= kHistLdsBytes;
    const bool lds_hist = open_level && tot_bytes + hist_bytes <= kHistLdsBytes;
    const size_t hsmem = static_cast<size_t>((lds_tot ? tot_bytes : 0) + (lds_hist ? hist_bytes : 0)) + 16;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(rf_hist_regress_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(hsmem)) != hipSuccess)
      return DAL_ERR_HIP;
    hipLaunchKernelGGL(rf_hist_regress_kernel, hgrid, dim3(256), hsmem, st, A, level, rows_per_block, lds_tot,
                       lds_hist);
    DAL_RETURN_IF_LAUNCH_FAILED();
    return DAL_OK;
  }

  // Leaf or best split of every node of the level from the workspace's sums.
  static int level_split(const RegJob& J, int level, hipStream_t st) {
    int64_t words = 0;
    const RegArgs A = rf_at_level(J, level, &words);
    const size_t ssmem = level < A.max_depth ? static_cast<size_t>(A.m) * A.hb * A.W * 8 : 16;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(rf_split_regress_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(ssmem)) != hipSuccess)
      return DAL_ERR_HIP;
    hipLaunchKernelGGL(rf_split_regress_kernel, dim3(1u << level, static_cast<unsigned>(A.T)), dim3(kSplitThreads),
                       ssmem, st, A, J.red, level);
    DAL_RETURN_IF_LAUNCH_FAILED();
    return DAL_OK;
  }

  static int finish(const RegJob& J, hipStream_t st) {
    const int64_t n_inner = (int64_t{1} << J.A.max_depth) - 1;
    hipLaunchKernelGGL(rf_finalize_regress_kernel,
                       dim3(static_cast<unsigned>(std::min<int64_t>(ceil_div(J.A.T * n_inner, 256), 4096))),
                       dim3(256), 0, st, J.A);
    DAL_RETURN_IF_LAUNCH_FAILED();
    return DAL_OK;
  }
};
using Regress = RfLadder<RegressTrainer>;

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" int dal_rf_find_splits_f64(const void* x, int x_dtype, int64_t n, int64_t d, int64_t ldx,
                                      const int64_t* sample_rows, int64_t n_sample, int32_t num_splits,
                                      double* thresholds, int32_t* n_splits, int32_t* dev_status,
                                      dal_stream_t stream) {
  if (!x || !thresholds || !n_splits || !dev_status) return DAL_ERR_ARG;
  if (x_dtype != DAL_X_F32 && x_dtype != DAL_X_F64) return DAL_ERR_ARG;
  if (n < 1 || d < 1 || ldx < d || n_sample < 1 || n_sample > max_sample(x_dtype)) return DAL_ERR_SHAPE;
  if (!sample_rows && n_sample > n) return DAL_ERR_SHAPE;
  if (num_splits < 0 || num_splits >= DAL_RF_MAX_SPLITS) return DAL_ERR_SHAPE;
  if (x_dtype == DAL_X_F64)
    return launch_find_splits(static_cast<const double*>(x), n, d, ldx, sample_rows, n_sample, num_splits,
                              thresholds, n_splits, dev_status, as_stream(stream));
  return launch_find_splits(static_cast<const float*>(x), n, d, ldx, sample_rows, n_sample, num_splits, thresholds,
                            n_splits, dev_status, as_stream(stream));
}

extern "C" int dal_rf_bin_rows(const void* x, int x_dtype, int64_t n, int64_t d, int64_t ldx,
                               const double* thresholds, const int32_t* n_splits, uint8_t* bins,
                               dal_stream_t stream) {
  if (!x || !thresholds || !n_splits || !bins) return DAL_ERR_ARG;
  if (x_dtype != DAL_X_F32 && x_dtype != DAL_X_F64) return DAL_ERR_ARG;
  if (n < 1 || d < 1 || ldx < d) return DAL_ERR_SHAPE;
  if (x_dtype == DAL_X_F64)
    return launch_bin(static_cast<const double*>(x), n, d, ldx, thresholds, n_splits, bins, as_stream(stream));
  return launch_bin(static_cast<const float*>(x), n, d, ldx, thresholds, n_splits, bins, as_stream(stream));
}

extern "C" size_t dal_rf_train_regressor_workspace_bytes(int64_t n, int32_t n_trees, int32_t max_depth, int32_t m,
                                                         int32_t num_splits, int32_t k_y, int32_t k_sq) {
  if (n < 1 || n_trees < 1 || max_depth < 1 || max_depth > DAL_RF_MAX_DEPTH || m < 1 || num_splits < 0 ||
      !limbs_ok(0, k_y) || !limbs_ok(0, k_sq))
    return 0;
  return reg_layout(n, n_trees, max_depth, m, num_splits + 2, 1 + k_y + k_sq).total;
}

extern "C" int dal_rf_train_regressor_begin(void* job, const uint8_t* bins, int64_t n_local, int64_t d,
                                            const double* y, const double* thresholds, const int32_t* n_splits,
                                            int32_t num_splits, const int32_t* weights,
                                            const int32_t* feature_subsets, int32_t m, int32_t n_trees,
                                            int32_t max_depth, int32_t min_instances, double min_info_gain,
                                            int32_t q_y, int32_t k_y, int32_t q_sq, int32_t k_sq,
                                            int32_t* out_feature, double* out_threshold, double* out_leaf, void* ws,
                                            size_t ws_bytes, dal_stream_t stream) {
  return Regress::begin(job, stream, bins, n_local, d, y, thresholds, n_splits, num_splits, weights, feature_subsets,
                        m, n_trees, max_depth, min_instances, min_info_gain, q_y, k_y, q_sq, k_sq, out_feature,
                        out_threshold, out_leaf, ws, ws_bytes);
}

extern "C" int dal_rf_train_regressor_level_stats(const void* job, int32_t level, dal_stream_t stream) {
  return Regress::level_stats(job, level, stream);
}

extern "C" int dal_rf_train_regressor_level_split(const void* job, int32_t level, dal_stream_t stream) {
  return Regress::level_split(job, level, stream);
}

extern "C" int dal_rf_train_regressor_finish(const void* job, dal_stream_t stream) {
  return Regress::finish(job, stream);
}

extern "C" int dal_rf_train_regressor_level_span(const void* job, int32_t level, void** ptr, int32_t* elem_type,
                                                 int64_t* count) {
  return Regress::level_span(job, level, ptr, elem_type, count);
}

extern "C" int dal_rf_train_regressor(const uint8_t* bins, int64_t n, int64_t d, const double* y,
                                      const double* thresholds, const int32_t* n_splits, int32_t num_splits,
                                      const int32_t* weights, const int32_t* feature_subsets, int32_t m,
                                      int32_t n_trees, int32_t max_depth, int32_t min_instances,
                                      double min_info_gain, int32_t q_y, int32_t k_y, int32_t q_sq, int32_t k_sq,
                                      int32_t* out_feature, double* out_threshold, double* out_leaf, void* ws,
                                      size_t ws_bytes, dal_stream_t stream) {
  return Regress::fit(stream, bins, n, d, y, thresholds, n_splits, num_splits, weights, feature_subsets, m, n_trees,
                      max_depth, min_instances, min_info_gain, q_y, k_y, q_sq, k_sq, out_feature, out_threshold,
                      out_leaf, ws, ws_bytes);
}
