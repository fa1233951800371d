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
#include <algorithm>
#include <cfloat>
#include <climits>

#include "common.hpp"
#include "rf_exact_sum.hpp"
#include "rf_train_shared.hpp"

namespace dal {
namespace {

constexpr int kSortThreads = 1024;
constexpr int kSplitThreads = 256;
constexpr int kSplitWaves = kSplitThreads / kWave;
constexpr int kRedBytes = 64;  // per node: kSplitWaves gains (fp64) then kSplitWaves pair indices (int32)
constexpr int64_t kHistLdsBytes = 64 * 1024;

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
  int64_t* tot;       // [T][2^l][W], ending where hist begins (reg_at_level)
  int32_t* out_feature;   // [T][n_inner]
  double* out_threshold;  // [T][n_inner]
  double* out_leaf;       // [T][n_leaf]
};

// The totals come right before the histogram and a level's totals are kept at
// the END of their piece: totals + histogram of a level are one span of int64
// (what a sharded fit sums over ranks: dal_rf_train_regressor_level_span).
struct RegLayout {
  size_t node, status, split_f, split_b, tot, hist, red, total;
};

RegLayout reg_layout(int64_t n, int64_t T, int max_depth, int64_t m, int64_t hb, int64_t W) {
  RegLayout L{};
  const int64_t n_inner = (int64_t{1} << max_depth) - 1;
  const int64_t split_nodes = int64_t{1} << (max_depth - 1);  // deepest level that is split
  size_t o = 0;
  auto take = [&](int64_t bytes) {
    const size_t at = o;
    o += static_cast<size_t>(round_up(bytes, 256));
    return at;
  };
  L.node = take(T * n * 4);
  L.status = take(T * (2 * n_inner + 1));
  L.split_f = take(T * n_inner * 4);
  L.split_b = take(T * n_inner * 4);
  L.tot = take(T * (n_inner + 1) * W * 8);
  L.hist = take(T * split_nodes * m * hb * W * 8);
  L.red = take(T * split_nodes * kRedBytes);
  L.total = o;
  return L;
}

// The job descriptor of the level steps (rf_train_shared.hpp has the
// classifiers'); A.tot holds the END of the totals piece (== A.hist).
struct RegJob {
  uint32_t magic;
  int32_t kind;
  unsigned char* red;
  RegArgs A;
};
static_assert(sizeof(RegJob) <= DAL_RF_JOB_BYTES, "DAL_RF_JOB_BYTES holds a regressor job");

// The level's view of the job's arguments; words = elements of the level's span from A.tot on.
RegArgs reg_at_level(const RegJob& J, int level, int64_t* words) {
  RegArgs A = J.A;
  const int64_t nodes = int64_t{1} << level;
  const int64_t tot_words = A.T * nodes * A.W;
  const int64_t hist_words = level < A.max_depth ? A.T * nodes * A.m * A.hb * A.W : 0;
  A.tot = A.hist - tot_words;
  *words = tot_words + hist_words;
  return A;
}

__device__ __forceinline__ int block_min_int(int v, int* red) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    int m = INT_MAX;
    for (int i = 0; i < static_cast<int>(blockDim.x >> 6); ++i) m = min(m, red[i]);
    red[0] = m;
  }
  __syncthreads();
  const int r = red[0];
  __syncthreads();
  return r;
}

// findSplitsForContinuousFeature over rows of X (float or double): one block
// per feature sorts the sample column in LDS in its own type and emits the
// thresholds as fp64 (the widening of an fp32 value is exact).  The steps are
// rf_find_splits_kernel's (rf_train.hip).
template <class X>
__global__ __launch_bounds__(kSortThreads) void rf_find_splits_f64_kernel(
    const X* __restrict__ x, int64_t n, int d, int64_t ldx, const int64_t* __restrict__ sample_rows, int n_s,
    int pow2, int num_splits, double* __restrict__ thresholds, int32_t* __restrict__ n_splits,
    int32_t* dev_status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  X* s = reinterpret_cast<X*>(smem);                                                // [pow2] sorted sample
  int* pos = reinterpret_cast<int*>(smem + static_cast<size_t>(pow2) * sizeof(X));  // [n_s] first row of distinct j
  int* red = pos + n_s;                                                             // [32] scan / reduction scratch
  const int f = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < pow2; i += kSortThreads) {
    X v = static_cast<X>(__builtin_inff());
    if (i < n_s) {
      const int64_t r = sample_rows ? sample_rows[i] : i;
      v = x[r * ldx + f];
    }
    s[i] = v;
  }
  __syncthreads();
  for (int k = 2; k <= pow2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < pow2; i += kSortThreads) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const X a = s[i], b = s[ixj];
          const bool up = (i & k) == 0;
          if ((a > b) == up) {
            s[i] = b;
            s[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  // distinct heads: each thread owns a contiguous chunk, block exclusive scan
  const int chunk = (n_s + kSortThreads - 1) / kSortThreads;
  const int i0 = min(tid * chunk, n_s), i1 = min(i0 + chunk, n_s);
  int cnt = 0;
  for (int i = i0; i < i1; ++i) cnt += (i == 0 || s[i] != s[i - 1]);
  int incl = cnt;
  const int lane = tid & 63, w = tid >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(incl, o);
    if (lane >= o) incl += y;
  }
  if (lane == 63) red[w] = incl;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int q = 0; q < kSortThreads / 64; ++q) {
      const int c = red[q];
      red[q] = run;
      run += c;
    }
    red[kSortThreads / 64] = run;
  }
  __syncthreads();
  int j = red[w] + incl - cnt;
  const int n_distinct = red[kSortThreads / 64];
  for (int i = i0; i < i1; ++i)
    if (i == 0 || s[i] != s[i - 1]) pos[j++] = i;
  __syncthreads();
  double* out = thresholds + static_cast<int64_t>(f) * DAL_RF_MAX_SPLITS;
  if (n_distinct <= num_splits) {
    for (int q = tid; q < n_distinct; q += kSortThreads) out[q] = static_cast<double>(s[pos[q]]);
    if (tid == 0) n_splits[f] = n_distinct;
    return;
  }
  // stride rule: the next threshold is uniq[j-1] for the first j >= start with
  // |cum[j-1] - target| < |cum[j] - target|; cum[j] = values <= uniq[j]
  const double stride = static_cast<double>(n_s) / static_cast<double>(num_splits + 1);
  double target = stride;
  int start = 1, emitted = 0;
  const int cap = min(num_splits + 1, DAL_RF_MAX_SPLITS);
  while (true) {
    int found = INT_MAX;
    for (int q = start + tid; q < n_distinct; q += kSortThreads) {
      const int prev = pos[q];                                // cum[q-1]
      const int cur = q + 1 < n_distinct ? pos[q + 1] : n_s;  // cum[q]
      if (fabs(static_cast<double>(prev) - target) < fabs(static_cast<double>(cur) - target)) {
        found = q;
        break;
      }
    }
    found = block_min_int(found, red);
    if (found == INT_MAX) break;
    if (emitted == cap) {
      if (tid == 0) atomicOr(dev_status, DAL_FLAG_RF_SPLITS);
      break;
    }
    if (tid == 0) out[emitted] = static_cast<double>(s[pos[found - 1]]);
    ++emitted;
    target += stride;
    start = found + 1;
  }
  if (tid == 0) n_splits[f] = emitted;
}

// bins[i][f] = #{thresholds_f < x[i][f]}, compared in fp64.
template <class X>
__global__ void rf_bin_f64_kernel(const X* __restrict__ x, int64_t n, int d, int64_t ldx,
                                  const double* __restrict__ thresholds, const int32_t* __restrict__ n_splits,
                                  uint8_t* __restrict__ bins) {
  const int64_t total = n * d;
  for (int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; e < total;
       e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t i = e / d;
    const int f = static_cast<int>(e - i * d);
    const double v = static_cast<double>(x[i * ldx + f]);
    const double* t = thresholds + static_cast<int64_t>(f) * DAL_RF_MAX_SPLITS;
    int lo = 0, hi = min(n_splits[f], DAL_RF_MAX_SPLITS);
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (t[mid] < v) lo = mid + 1;
      else hi = mid;
    }
    bins[e] = static_cast<uint8_t>(lo);
  }
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
  const int n_inner = (1 << A.max_depth) - 1;
  const int span = 1 << (A.max_depth - level);
  const int first_leaf = (h + 1) * span - 1 - n_inner;
  const int64_t count = gt[0];
  double v = 0.0;
  if (count != 0) v = exact::to_double([&](int j) { return gt[1 + j]; }, A.k_y, A.q_y) / static_cast<double>(count);
  double* out = A.out_leaf + static_cast<int64_t>(t) * (n_inner + 1) + first_leaf;
  for (int q = 0; q < span; ++q) out[q] = v;
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
  for (int q = tid; q < A.m * W; q += kSplitThreads) {
    const int nb = min(A.n_splits[sub[q / W]] + 1, hb);
    int64_t* row = cum + q * hb;
    int64_t a = 0;
    for (int b = 0; b < nb; ++b) {
      a += row[b];
      row[b] = a;
    }
  }
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
    fill_leaf_regress(A, t, h, level, gt);
    A.split_f[static_cast<int64_t>(t) * n_inner + h] = -1;
    return;
  }
  const int s = best_p / A.kmax, k = best_p - s * A.kmax;
  double li = 0.0, ri = 0.0;
  split_gain_regress(A, cum + s * W * hb + k, gt, tc, parent_imp, &li, &ri);
  A.split_f[static_cast<int64_t>(t) * n_inner + h] = sub[s];
  A.split_b[static_cast<int64_t>(t) * n_inner + h] = k;
  const bool child_leaf = level + 1 == A.max_depth;
  st[2 * h + 1] = (child_leaf || li == 0.0) ? kLeaf : kOpen;
  st[2 * h + 2] = (child_leaf || ri == 0.0) ? kLeaf : kOpen;
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

__global__ void rf_open_roots_kernel(uint8_t* status, int T, int64_t n_all) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < T) status[static_cast<int64_t>(t) * n_all] = kOpen;
}

bool limbs_ok(int32_t q, int32_t k) { return k >= 1 && k <= DAL_RF_REG_MAX_LIMBS && q >= -1074 && q <= 1023; }

int64_t max_sample(int x_dtype) {
  return x_dtype == DAL_X_F64 ? DAL_RF_MAX_SPLIT_SAMPLE_F64 : DAL_RF_MAX_SPLIT_SAMPLE;
}

template <class X>
int launch_find_splits(const X* x, int64_t n, int64_t d, int64_t ldx, const int64_t* sample_rows, int64_t n_sample,
                       int32_t num_splits, double* thresholds, int32_t* n_splits, int32_t* dev_status,
                       hipStream_t st) {
  int pow2 = 1;
  while (pow2 < n_sample) pow2 <<= 1;
  const size_t smem = static_cast<size_t>(pow2) * sizeof(X) + static_cast<size_t>(n_sample) * 4 + 32 * 4;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(rf_find_splits_f64_kernel<X>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem)) != hipSuccess)
    return DAL_ERR_HIP;
  hipLaunchKernelGGL(rf_find_splits_f64_kernel<X>, dim3(static_cast<unsigned>(d)), dim3(kSortThreads), smem, st, x,
                     n, static_cast<int>(d), ldx, sample_rows, static_cast<int>(n_sample), pow2, num_splits,
                     thresholds, n_splits, dev_status);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

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
  const dim3 grid(static_cast<unsigned>(std::min<int64_t>(ceil_div(n * d, 256), 4096)));
  if (x_dtype == DAL_X_F64)
    hipLaunchKernelGGL(rf_bin_f64_kernel<double>, grid, dim3(256), 0, as_stream(stream),
                       static_cast<const double*>(x), n, static_cast<int>(d), ldx, thresholds, n_splits, bins);
  else
    hipLaunchKernelGGL(rf_bin_f64_kernel<float>, grid, dim3(256), 0, as_stream(stream),
                       static_cast<const float*>(x), n, static_cast<int>(d), ldx, thresholds, n_splits, bins);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

extern "C" size_t dal_rf_train_regressor_workspace_bytes(int64_t n, int32_t n_trees, int32_t max_depth, int32_t m,
                                                         int32_t num_splits, int32_t k_y, int32_t k_sq) {
  if (n < 1 || n_trees < 1 || max_depth < 1 || max_depth > DAL_RF_MAX_DEPTH || m < 1 || num_splits < 0 ||
      !limbs_ok(0, k_y) || !limbs_ok(0, k_sq))
    return 0;
  return reg_layout(n, n_trees, max_depth, m, num_splits + 2, 1 + k_y + k_sq).total;
}

namespace dal {
namespace {

// The argument checks of dal_rf_train_regressor over n >= min_n rows, the
// workspace layout, the job, then every tree's root open and every other
// node absent.  bins, y and weights may be null for a job of no rows.  *Jp
// is the job; it is also copied to the caller's descriptor `job` (nullable)
// before the first device call.
int regress_begin(RegJob* Jp, void* job, const uint8_t* bins, int64_t n, int64_t d, const double* y, const double* thresholds,
                  const int32_t* n_splits, int32_t num_splits, const int32_t* weights,
                  const int32_t* feature_subsets, int32_t m, int32_t n_trees, int32_t max_depth,
                  int32_t min_instances, double min_info_gain, int32_t q_y, int32_t k_y, int32_t q_sq, int32_t k_sq,
                  int32_t* out_feature, double* out_threshold, double* out_leaf, void* ws, size_t ws_bytes,
                  int64_t min_n, hipStream_t st) {
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
  const RegLayout L = reg_layout(n, n_trees, max_depth, m, hb, W);
  if (ws_bytes < L.total || reinterpret_cast<uintptr_t>(ws) % 256) return DAL_ERR_SHAPE;
  unsigned char* w = static_cast<unsigned char*>(ws);
  RegJob& J = *Jp;
  J = RegJob{};
  J.magic = kRfJobMagic;
  J.kind = kRfJobRegress;
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

  const int64_t n_inner = (int64_t{1} << max_depth) - 1;
  // root open, everything else absent
  if (hipMemsetAsync(A.status, 0, static_cast<size_t>(n_trees) * (2 * n_inner + 1), st) != hipSuccess)
    return DAL_ERR_HIP;
  hipLaunchKernelGGL(rf_open_roots_kernel, dim3(static_cast<unsigned>(ceil_div(n_trees, 256))), dim3(256), 0, st,
                     A.status, n_trees, 2 * n_inner + 1);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

// Zero the level's totals and histogram, then add the job's rows to them.
int regress_level_stats(const RegJob& J, int level, hipStream_t st) {
  int64_t words = 0;
  const RegArgs A = reg_at_level(J, level, &words);
  if (hipMemsetAsync(A.tot, 0, static_cast<size_t>(words) * 8, st) != hipSuccess) return DAL_ERR_HIP;
  if (A.n == 0) return DAL_OK;
  const int64_t nodes = int64_t{1} << level;
  const bool open_level = level < A.max_depth;
  const int64_t tot_bytes = nodes * A.W * 8;
  const int64_t hist_bytes = open_level ? nodes * A.m * A.hb * A.W * 8 : 0;
  const int rows_per_block = 1024;
  const dim3 hgrid(static_cast<unsigned>(ceil_div(A.n, rows_per_block)), static_cast<unsigned>(A.T));
  // the classifiers' budget: totals + level histogram within 64 KiB, else global atomics
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
int regress_level_split(const RegJob& J, int level, hipStream_t st) {
  int64_t words = 0;
  const RegArgs A = reg_at_level(J, level, &words);
  const size_t ssmem = level < A.max_depth ? static_cast<size_t>(A.m) * A.hb * A.W * 8 : 16;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(rf_split_regress_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(ssmem)) != hipSuccess)
    return DAL_ERR_HIP;
  hipLaunchKernelGGL(rf_split_regress_kernel, dim3(1u << level, static_cast<unsigned>(A.T)), dim3(kSplitThreads),
                     ssmem, st, A, J.red, level);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

int regress_finish(const RegJob& J, hipStream_t st) {
  const int64_t n_inner = (int64_t{1} << J.A.max_depth) - 1;
  hipLaunchKernelGGL(rf_finalize_regress_kernel,
                     dim3(static_cast<unsigned>(std::min<int64_t>(ceil_div(J.A.T * n_inner, 256), 4096))), dim3(256),
                     0, st, J.A);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

}  // namespace
}  // namespace dal

extern "C" int dal_rf_train_regressor_begin(void* job, const uint8_t* bins, int64_t n_local, int64_t d,
                                            const double* y, const double* thresholds, const int32_t* n_splits,
                                            int32_t num_splits, const int32_t* weights,
                                            const int32_t* feature_subsets, int32_t m, int32_t n_trees,
                                            int32_t max_depth, int32_t min_instances, double min_info_gain,
                                            int32_t q_y, int32_t k_y, int32_t q_sq, int32_t k_sq,
                                            int32_t* out_feature, double* out_threshold, double* out_leaf, void* ws,
                                            size_t ws_bytes, dal_stream_t stream) {
  RegJob J;
  if (!job) return DAL_ERR_ARG;
  return regress_begin(&J, job, bins, n_local, d, y, thresholds, n_splits, num_splits, weights, feature_subsets, m,
                       n_trees, max_depth, min_instances, min_info_gain, q_y, k_y, q_sq, k_sq, out_feature,
                       out_threshold, out_leaf, ws, ws_bytes, 0, as_stream(stream));
}

extern "C" int dal_rf_train_regressor_level_stats(const void* job, int32_t level, dal_stream_t stream) {
  RegJob J;
  if (const int rc = rf_job_load(job, kRfJobRegress, level, &J)) return rc;
  return regress_level_stats(J, level, as_stream(stream));
}

extern "C" int dal_rf_train_regressor_level_split(const void* job, int32_t level, dal_stream_t stream) {
  RegJob J;
  if (const int rc = rf_job_load(job, kRfJobRegress, level, &J)) return rc;
  return regress_level_split(J, level, as_stream(stream));
}

extern "C" int dal_rf_train_regressor_finish(const void* job, dal_stream_t stream) {
  RegJob J;
  if (const int rc = rf_job_load(job, kRfJobRegress, 0, &J)) return rc;
  return regress_finish(J, as_stream(stream));
}

extern "C" int dal_rf_train_regressor_level_span(const void* job, int32_t level, void** ptr, int32_t* elem_type,
                                                 int64_t* count) {
  RegJob J;
  if (!ptr || !elem_type || !count) return DAL_ERR_ARG;
  if (const int rc = rf_job_load(job, kRfJobRegress, level, &J)) return rc;
  const RegArgs A = reg_at_level(J, level, count);
  *ptr = A.tot;
  *elem_type = DAL_RF_SPAN_I64;
  return DAL_OK;
}

extern "C" int dal_rf_train_regressor(const uint8_t* bins, int64_t n, int64_t d, const double* y,
                                      const double* thresholds, const int32_t* n_splits, int32_t num_splits,
                                      const int32_t* weights, const int32_t* feature_subsets, int32_t m,
                                      int32_t n_trees, int32_t max_depth, int32_t min_instances,
                                      double min_info_gain, int32_t q_y, int32_t k_y, int32_t q_sq, int32_t k_sq,
                                      int32_t* out_feature, double* out_threshold, double* out_leaf, void* ws,
                                      size_t ws_bytes, dal_stream_t stream) {
  RegJob J;
  hipStream_t st = as_stream(stream);
  if (const int rc = regress_begin(&J, nullptr, bins, n, d, y, thresholds, n_splits, num_splits, weights, feature_subsets, m,
                                   n_trees, max_depth, min_instances, min_info_gain, q_y, k_y, q_sq, k_sq,
                                   out_feature, out_threshold, out_leaf, ws, ws_bytes, 1, st))
    return rc;
  for (int level = 0; level <= max_depth; ++level) {
    if (const int rc = regress_level_stats(J, level, st)) return rc;
    if (const int rc = regress_level_split(J, level, st)) return rc;
  }
  return regress_finish(J, st);
}
