// What the three forest trainers' kernels share (rf_train.hip, the binary
// Gini trainer; rf_train_multi.hip, C classes; rf_train_regress.hip,
// variance): the threshold search, the binning, a row's routing from one level
// to the next, the pieces of a split kernel that do not depend on the
// impurity -- leaf span, per-series prefix sums, the first-maximum reduction
// and its four-wave exchange, the commit of a split -- and the entry ladder
// over the level steps.  One definition each; every file instantiates what it
// uses.  Args is RfArgs or the regressor's RegArgs: the helpers read only the
// fields the two have in common.  scripts/isa_diff.py against the commit
// before compares every kernel (profiles/rf_train_shared/).
#pragma once

#include <algorithm>
#include <cfloat>
#include <climits>

#include "common.hpp"
#include "rf_train_shared.hpp"

namespace dal {
namespace {

constexpr int kSortThreads = 1024;

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
// per feature sorts the sample column in LDS in its own type, finds the
// distinct values and their cumulative counts and emits the thresholds as Th
// (the widening of an fp32 value to fp64 is exact).
template <class X, class Th>
__global__ __launch_bounds__(kSortThreads) void rf_find_splits_kernel(
    const X* __restrict__ x, int64_t n, int d, int64_t ldx, const int64_t* __restrict__ sample_rows, int n_s,
    int pow2, int num_splits, Th* __restrict__ thresholds, int32_t* __restrict__ n_splits, int32_t* dev_status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  X* s = reinterpret_cast<X*>(smem);                                                // [pow2] sorted sample
  int* pos = reinterpret_cast<int*>(smem + static_cast<size_t>(pow2) * sizeof(X));  // [n_s] first position of distinct j
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
  // wave-inclusive scan, then across the 16 waves
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
  Th* out = thresholds + static_cast<int64_t>(f) * DAL_RF_MAX_SPLITS;
  if (n_distinct <= num_splits) {
    for (int q = tid; q < n_distinct; q += kSortThreads) out[q] = static_cast<Th>(s[pos[q]]);
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
    if (tid == 0) out[emitted] = static_cast<Th>(s[pos[found - 1]]);
    ++emitted;
    target += stride;
    start = found + 1;
  }
  if (tid == 0) n_splits[f] = emitted;
}

// The launch of the threshold search; the entries keep their argument checks
// and sample caps.  DAL_OK or DAL_ERR_HIP.
template <class X, class Th>
int launch_find_splits(const X* x, int64_t n, int64_t d, int64_t ldx, const int64_t* sample_rows, int64_t n_sample,
                       int32_t num_splits, Th* thresholds, int32_t* n_splits, int32_t* dev_status, hipStream_t st) {
  int pow2 = 1;
  while (pow2 < n_sample) pow2 <<= 1;
  const size_t smem = static_cast<size_t>(pow2) * sizeof(X) + static_cast<size_t>(n_sample) * 4 + 32 * 4;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(rf_find_splits_kernel<X, Th>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem)) != hipSuccess)
    return DAL_ERR_HIP;
  hipLaunchKernelGGL((rf_find_splits_kernel<X, Th>), dim3(static_cast<unsigned>(d)), dim3(kSortThreads), smem, st, x,
                     n, static_cast<int>(d), ldx, sample_rows, static_cast<int>(n_sample), pow2, num_splits,
                     thresholds, n_splits, dev_status);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

// bins[i][f] = #{thresholds_f < x[i][f]}, compared in Th (lower bound; an
// equal threshold gives its own index, as Arrays.binarySearch does).  A
// threshold count past the table's row is read as the row's length.
template <class X, class Th>
__global__ void rf_bin_kernel(const X* __restrict__ x, int64_t n, int d, int64_t ldx,
                              const Th* __restrict__ thresholds, const int32_t* __restrict__ n_splits,
                              uint8_t* __restrict__ bins) {
  const int64_t total = n * d;
  for (int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; e < total;
       e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t i = e / d;
    const int f = static_cast<int>(e - i * d);
    const Th v = static_cast<Th>(x[i * ldx + f]);
    const Th* t = thresholds + static_cast<int64_t>(f) * DAL_RF_MAX_SPLITS;
    int lo = 0, hi = min(n_splits[f], DAL_RF_MAX_SPLITS);
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (t[mid] < v) lo = mid + 1;
      else hi = mid;
    }
    bins[e] = static_cast<uint8_t>(lo);
  }
}

template <class X, class Th>
int launch_bin(const X* x, int64_t n, int64_t d, int64_t ldx, const Th* thresholds, const int32_t* n_splits,
               uint8_t* bins, hipStream_t st) {
  hipLaunchKernelGGL((rf_bin_kernel<X, Th>), dim3(static_cast<unsigned>(std::min<int64_t>(ceil_div(n * d, 256), 4096))),
                     dim3(256), 0, st, x, n, static_cast<int>(d), ldx, thresholds, n_splits, bins);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

// ------------------------------------------------------------ histogram --
// Row i of tree t (of positive weight: the kernel's test) from level - 1 to
// level: its heap index at this level, stored to A.node, or kSettled with
// live false for a row settled before or one whose node became a leaf
// (settled here).  live and not a test of h: the kernels' `continue` then
// compiles to the branches it had but for one -- the "became a leaf" flag is
// tested again instead of kept in a mask (DESIGN.md has the counts); with the
// weight read in here as well the regressor's kernel took two more VGPRs.
constexpr int kSettled = -1;
struct Routed {
  int h;
  bool live;
};
template <class Args>
__device__ __forceinline__ Routed route_row(const Args& A, int t, int64_t i, int level, int n_inner) {
  int32_t* nd = A.node + static_cast<int64_t>(t) * A.n + i;
  int h = 0;
  if (level > 0) {
    const int hp = *nd;
    if (hp < 0) return {kSettled, false};
    const int f = A.split_f[static_cast<int64_t>(t) * n_inner + hp];
    if (f < 0) {  // the row's node became a leaf
      *nd = kSettled;
      return {kSettled, false};
    }
    const int b = A.bins[i * A.d + f];
    h = 2 * hp + 1 + (b > A.split_b[static_cast<int64_t>(t) * n_inner + hp] ? 1 : 0);
  }
  *nd = h;
  return {h, true};
}

// ---------------------------------------------------------------- split --
// The leaves of node h's heap subtree (h at `level`) in tree t's row of
// out_leaf.  (The fill loop over them and a leaf's split_f = -1 stay in the
// kernels: as helpers they moved the split kernels' instruction counts.)
struct LeafSpan {
  int64_t first;
  int count;
};
template <class Args>
__device__ __forceinline__ LeafSpan leaf_span(const Args& A, int t, int h, int level) {
  const int n_inner = (1 << A.max_depth) - 1;
  const int span = 1 << (A.max_depth - level);
  const int first_leaf = (h + 1) * span - 1 - n_inner;
  return {static_cast<int64_t>(t) * (n_inner + 1) + first_leaf, span};
}
// cum [m][per_slot][hb] in LDS: every (slot, word) series becomes its prefix
// sums over the slot's feature's bins, a series per thread (tid: threadIdx.x).
template <class Args, class Word>
__device__ __forceinline__ void prefix_sum_series(const Args& A, Word* cum, int per_slot, const int32_t* sub, int tid) {
  for (int q = tid; q < A.m * per_slot; q += kSplitThreads) {
    const int nb = min(A.n_splits[sub[q / per_slot]] + 1, A.hb);
    Word* row = cum + q * A.hb;
    Word a = 0;
    for (int b = 0; b < nb; ++b) {
      a += row[b];
      row[b] = a;
    }
  }
}

// Lexicographic first maximum over (gain descending, pair index ascending).
__device__ __forceinline__ void first_max(double& best, int& best_p, double og, int op) {
  if (og > best || (og == best && op < best_p)) {
    best = og;
    best_p = op;
  }
}
__device__ __forceinline__ void wave_first_max(double& best, int& best_p) {
  for (int o = 32; o > 0; o >>= 1) {
    const double og = __shfl_xor(best, o);
    const int op = __shfl_xor(best_p, o);
    first_max(best, best_p, og, op);
  }
}
// ... then over the block's kSplitWaves waves through r, the node's kRedBytes
// of workspace (the LDS is the histogram's up to its last byte): thread 0
// returns with the block's.  Every thread of the block calls (tid:
// threadIdx.x).  The wave leaders' stores go to global memory: each leader
// waits for its own to have left the wave before it arrives at the barrier
// that thread 0 reads them after.
__device__ __forceinline__ void block_first_max(unsigned char* r, double& best, int& best_p, int tid) {
  double* red_g = reinterpret_cast<double*>(r);
  int* red_p = reinterpret_cast<int*>(r + kSplitWaves * 8);
  if ((tid & (kWave - 1)) == 0) {
    red_g[tid / kWave] = best;
    red_p[tid / kWave] = best_p;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores have left this wave before the barrier
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < kSplitWaves; ++w) first_max(best, best_p, red_g[w], red_p[w]);
}
// Node h splits on feature f at split k; li, ri: the children's impurities
// (a pure child is a leaf, as is every child at max_depth).
template <class Args>
__device__ __forceinline__ void commit_split(const Args& A, uint8_t* st, int t, int h, int level, int n_inner, int f,
                                             int k, double li, double ri) {
  A.split_f[static_cast<int64_t>(t) * n_inner + h] = f;
  A.split_b[static_cast<int64_t>(t) * n_inner + h] = k;
  const bool child_leaf = level + 1 == A.max_depth;
  st[2 * h + 1] = (child_leaf || li == 0.0) ? kLeaf : kOpen;
  st[2 * h + 2] = (child_leaf || ri == 0.0) ? kLeaf : kOpen;
}

// ---------------------------------------------------------- entry ladder --
// The level-step entries and the whole fit of one trainer.  Tr supplies
//   Job, kKind
//   begin(Job*, void* job, int64_t min_n, hipStream_t, args...)  checks, job, bins / reset
//   level_stats(const Job&, level, st), level_split(const Job&, level, st), finish(const Job&, st)
// A job is refused by the entries of another kind (rf_job_load).
template <class Tr>
struct RfLadder {
  using Job = typename Tr::Job;
  template <class... Args>
  static int begin(void* job, dal_stream_t stream, Args... args) {
    Job J;
    if (!job) return DAL_ERR_ARG;
    return Tr::begin(&J, job, 0, as_stream(stream), args...);
  }
  static int level_stats(const void* job, int32_t level, dal_stream_t stream) {
    Job J;
    if (const int rc = rf_job_load(job, Tr::kKind, level, &J)) return rc;
    return Tr::level_stats(J, level, as_stream(stream));
  }
  static int level_split(const void* job, int32_t level, dal_stream_t stream) {
    Job J;
    if (const int rc = rf_job_load(job, Tr::kKind, level, &J)) return rc;
    return Tr::level_split(J, level, as_stream(stream));
  }
  static int finish(const void* job, dal_stream_t stream) {
    Job J;
    if (const int rc = rf_job_load(job, Tr::kKind, 0, &J)) return rc;
    return Tr::finish(J, as_stream(stream));
  }
  static int level_span(const void* job, int32_t level, void** ptr, int32_t* elem_type, int64_t* count) {
    Job J;
    if (!ptr || !elem_type || !count) return DAL_ERR_ARG;
    if (const int rc = rf_job_load(job, Tr::kKind, level, &J)) return rc;
    const auto A = rf_at_level(J, level, count);
    *ptr = A.tot;
    *elem_type = sizeof(*A.tot) == 8 ? DAL_RF_SPAN_I64 : DAL_RF_SPAN_I32;
    return DAL_OK;
  }
  template <class... Args>
  static int fit(dal_stream_t stream, Args... args) {
    Job J;
    hipStream_t st = as_stream(stream);
    if (const int rc = Tr::begin(&J, nullptr, 1, st, args...)) return rc;
    for (int level = 0; level <= J.A.max_depth; ++level) {
      if (const int rc = Tr::level_stats(J, level, st)) return rc;
      if (const int rc = Tr::level_split(J, level, st)) return rc;
    }
    return Tr::finish(J, st);
  }
};

}  // namespace
}  // namespace dal
