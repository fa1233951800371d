// "Learning Active Learning" query scores from the forest votes.
//
// Reference: lal_direct_mllib_implementation/classes/active_learner.py:240-343
// (ActiveLearnerLAL.selectNext).  Its five features per unlabeled row are
//   f1 = v / T (:280), f2 = getSD(v, T) (:232-236, :283)   -- functions of the vote count v
//   f3 = positives / nLabeled (:288), f6 = mean of f2 over the unlabeled rows (:292),
//   f8 = nLabeled (:296)                                    -- per-step scalars
// so the regressor's prediction (:319) depends on a row through v alone: a
// look-up table of T + 1 entries.  The step is
//   votes (dal_forest_score) -> dal_vote_histogram -> (all-reduce when sharded)
//   -> dal_lal_rows -> dal_forest_regress on T + 1 rows -> dal_votes_rescore -> dal_topk
// all stream-ordered; nothing waits on the host.  The kernels here are the
// small ones: integers, and fp64 add / multiply / divide in the fixed order
// include/dal.h states.
#include "common.hpp"

namespace dal {
namespace {

constexpr int kLalThreads = 256;
constexpr int kHistRowsPerThread = 16;

// Vote histogram of the candidate rows.  A wave whose live lanes all hold one
// vote count (a confident forest: most rows at 0 or T) adds its lane count
// once; otherwise each lane adds to the block's LDS counters.  One int64
// global atomic per occupied bin per block: integer adds, exact in any order.
__global__ __launch_bounds__(kLalThreads) void vote_histogram_kernel(const int32_t* __restrict__ votes,
                                                                     const uint8_t* __restrict__ flags, int64_t n,
                                                                     int n_bins, unsigned long long* hist) {
  extern __shared__ unsigned int s_hist[];
  for (int b = threadIdx.x; b < n_bins; b += kLalThreads) s_hist[b] = 0u;
  __syncthreads();
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kLalThreads;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kLalThreads;
  for (int64_t base = first; base < n; base += stride) {  // (block-uniform trip count)
    const int64_t i = base + threadIdx.x;
    int v = -1;
    if (i < n && (!flags || (flags[i] & DAL_ROW_CANDIDATE))) v = votes[i];
    const bool counted = v >= 0 && v < n_bins;  // (a vote outside [0, T] is counted nowhere)
    const unsigned long long mask = __ballot(counted);
    if (mask == 0ull) continue;  // wave-uniform
    const int lead = __ffsll(static_cast<long long>(mask)) - 1;
    const int v0 = __shfl(v, lead);
    if (__ballot(counted && v == v0) == mask) {
      if ((threadIdx.x & 63) == lead) atomicAdd(&s_hist[v0], static_cast<unsigned>(__popcll(mask)));
    } else if (counted) {
      atomicAdd(&s_hist[v], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < n_bins; b += kLalThreads)
    if (s_hist[b]) atomicAdd(&hist[b], static_cast<unsigned long long>(s_hist[b]));
}

// rows[v] = {f1[v], f2[v], f3, f6, f8}, v = 0..T, with
//   f6 = (((0.0 + (double)h[0] * f2[0]) + (double)h[1] * f2[1]) + ...) / (double)nU,
//   nU = sum of the bins (int64).  The chain is T + 1 dependent adds: thread 0
// runs it over LDS copies, the block writes the rows.
__global__ __launch_bounds__(kLalThreads) void lal_rows_kernel(const int64_t* __restrict__ hist,
                                                               const double* __restrict__ f1,
                                                               const double* __restrict__ f2, int n_bins, double f3,
                                                               double f8, double* rows) {
  extern __shared__ __attribute__((aligned(8))) unsigned char smem[];
  double* s_term = reinterpret_cast<double*>(smem);  // (double)h[v] * f2[v]
  long long* s_h = reinterpret_cast<long long*>(smem) + n_bins;
  __shared__ double s_f6;
  for (int v = threadIdx.x; v < n_bins; v += kLalThreads) {
    const long long h = hist[v];
    s_h[v] = h;
    s_term[v] = __dmul_rn(static_cast<double>(h), f2[v]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long nu = 0;
    double s = 0.0;
    for (int v = 0; v < n_bins; ++v) {
      nu += s_h[v];
      s = __dadd_rn(s, s_term[v]);
    }
    s_f6 = nu > 0 ? s / static_cast<double>(nu) : __builtin_nan("");
  }
  __syncthreads();
  const double f6 = s_f6;
  for (int v = threadIdx.x; v < n_bins; v += kLalThreads) {
    double* r = rows + 5 * static_cast<int64_t>(v);
    r[0] = f1[v];
    r[1] = f2[v];
    r[2] = f3;
    r[3] = f6;
    r[4] = f8;
  }
}

// scores[i] = lut[votes[i]] and the score key dal_forest_score writes for it.
__global__ __launch_bounds__(kLalThreads) void votes_rescore_kernel(const int32_t* __restrict__ votes,
                                                                    const uint8_t* __restrict__ flags, int64_t n,
                                                                    const double* __restrict__ lut, int n_bins,
                                                                    int order, double* scores,
                                                                    unsigned long long* keys) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kLalThreads + threadIdx.x;
  if (i >= n) return;
  const int v = votes[i];
  const double s = v >= 0 && v < n_bins ? lut[v] : __builtin_nan("");  // (a vote outside [0, T]: no stray read)
  const uint8_t fl = flags ? flags[i] : static_cast<uint8_t>(DAL_ROW_CANDIDATE);
  scores[i] = s;
  keys[i] = (fl & DAL_ROW_CANDIDATE) ? score_key(s, order) : DAL_KEY_NONE;
}

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" int dal_vote_histogram(const int32_t* votes, const uint8_t* row_flags, int64_t n, int32_t n_trees,
                                  int64_t* hist, dal_stream_t stream) {
  if (!votes || !hist) return DAL_ERR_ARG;
  if (n_trees < 1 || n_trees > DAL_LAL_MAX_TREES) return DAL_ERR_UNSUPPORTED;
  if (n < 0 || n > (int64_t{1} << 40)) return DAL_ERR_SHAPE;
  if (n == 0) return DAL_OK;
  const int n_bins = n_trees + 1;
  // at most 2^40 / 4096 rows per block: the 32-bit LDS counters cannot wrap
  int64_t blocks = ceil_div(n, static_cast<int64_t>(kLalThreads) * kHistRowsPerThread);
  blocks = blocks > 4096 ? 4096 : blocks;
  hipLaunchKernelGGL(vote_histogram_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kLalThreads),
                     n_bins * sizeof(unsigned int), as_stream(stream), votes, row_flags, n, n_bins,
                     reinterpret_cast<unsigned long long*>(hist));
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

extern "C" int dal_lal_rows(const int64_t* hist, const double* f1, const double* f2, int32_t n_trees, double f3,
                            double f8, double* rows, dal_stream_t stream) {
  if (!hist || !f1 || !f2 || !rows) return DAL_ERR_ARG;
  if (n_trees < 1 || n_trees > DAL_LAL_MAX_TREES) return DAL_ERR_UNSUPPORTED;
  const int n_bins = n_trees + 1;
  hipLaunchKernelGGL(lal_rows_kernel, dim3(1), dim3(kLalThreads), n_bins * 16, as_stream(stream), hist, f1, f2,
                     n_bins, f3, f8, rows);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

extern "C" int dal_votes_rescore(const int32_t* votes, const uint8_t* row_flags, int64_t n, const double* lut,
                                 int32_t n_trees, int order, double* scores, uint64_t* keys, dal_stream_t stream) {
  if (!votes || !lut || !scores || !keys) return DAL_ERR_ARG;
  if (order != DAL_ASCENDING && order != DAL_DESCENDING) return DAL_ERR_ARG;
  if (n_trees < 1) return DAL_ERR_SHAPE;
  if (n < 0 || ceil_div(n, kLalThreads) > INT32_MAX) return DAL_ERR_SHAPE;
  if (n == 0) return DAL_OK;
  hipLaunchKernelGGL(votes_rescore_kernel, dim3(static_cast<unsigned>(ceil_div(n, kLalThreads))), dim3(kLalThreads), 0,
                     as_stream(stream), votes, row_flags, n, lut, n_trees + 1, order, scores,
                     reinterpret_cast<unsigned long long*>(keys));
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}
