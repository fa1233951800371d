// The exact sum of squared errors of a regressor's predictions:
//   testMSE = sum (label - prediction)^2 / count
//   (lal_direct_mllib_implementation/mllib/mllib_random_forest_regressor.py:48,
//   save_regression_model.py:51, mllib_randomforest_regression_lal_randomtree_
//   dataset.py:48): the one quality figure the LAL regressor gets.
// Spark sums the squares in partition arrival order; here s_i = fl(fl(y_i -
// pred_i)^2) is summed as an exact integer in 31-bit limbs (rf_exact_sum.hpp)
// with 64-bit integer atomics, so the sum is the same words for every row
// order, grid and chunking, and the host rounds the quotient once (dal.metrics).
//
//   format      atomic min of the lowest set bit's exponent and atomic max of
//               the exponent above the highest set bit over the nonzero s_i
//               (one pair per block), a status bit for a non-finite s_i;
//   accumulate  cells[k] += the k limbs of every s_i for the quantum 2^q: a
//               thread keeps its int64 words in registers over a strided set of
//               rows, a wave sums them by shuffles, the block through LDS, one
//               global atomic per (block, nonzero word).
#include "common.hpp"
#include "sq_error_exact.hpp"

namespace dal {
namespace {

constexpr int kSqThreads = 256;
constexpr int kSqWaves = kSqThreads / 64;
constexpr int kSqRowsPerThread = 8;
constexpr int kSqMaxBlocks = 2048;  // 8 per CU

int64_t sq_blocks(int64_t n) {
  const int64_t b = ceil_div(n, static_cast<int64_t>(kSqThreads) * kSqRowsPerThread);
  return b > kSqMaxBlocks ? kSqMaxBlocks : b;
}

__global__ __launch_bounds__(kSqThreads) void sq_error_format_kernel(const double* __restrict__ pred,
                                                                     const double* __restrict__ y, int64_t n,
                                                                     int32_t* low, int32_t* top,
                                                                     int32_t* dev_status) {
  __shared__ int s_low[kSqWaves], s_top[kSqWaves];
  int lo = sqerr::kNoLow, hi = sqerr::kNoTop, bad = 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kSqThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kSqThreads + threadIdx.x; i < n; i += stride) {
    const double s = sqerr::squared_error(pred[i], y[i]);
    if (!sqerr::finite_f64(s)) {
      bad = 1;
      continue;
    }
    const exact::Parts p = exact::parts(s);
    if (!p.mant) continue;
    lo = min(lo, sqerr::low_exponent(p));
    hi = max(hi, sqerr::top_exponent(p));
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o));
    hi = max(hi, __shfl_xor(hi, o));
  }
  if ((threadIdx.x & 63) == 0) {
    s_low[threadIdx.x >> 6] = lo;
    s_top[threadIdx.x >> 6] = hi;
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    if (bad) atomicOr(dev_status, DAL_FLAG_NONFINITE);
    for (int w = 1; w < kSqWaves; ++w) {
      lo = min(lo, s_low[w]);
      hi = max(hi, s_top[w]);
    }
    if (lo != sqerr::kNoLow) atomicMin(low, lo);
    if (hi != sqerr::kNoTop) atomicMax(top, hi);
  }
}

__global__ __launch_bounds__(kSqThreads) void sq_error_accumulate_kernel(const double* __restrict__ pred,
                                                                         const double* __restrict__ y, int64_t n,
                                                                         int q, int k, int64_t* cells) {
  __shared__ long long s_part[kSqWaves][exact::kMaxLimbs];
  long long a[exact::kMaxLimbs];  // fixed indices: registers
#pragma unroll
  for (int j = 0; j < exact::kMaxLimbs; ++j) a[j] = 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kSqThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kSqThreads + threadIdx.x; i < n; i += stride) {
    const double s = sqerr::squared_error(pred[i], y[i]);
    if (!sqerr::finite_f64(s)) continue;  // (refused by the format pass)
    const exact::Parts p = exact::parts(s);
#pragma unroll
    for (int j = 0; j < exact::kMaxLimbs; ++j)
      if (j < k) a[j] += exact::limb(p, q, j);
  }
#pragma unroll
  for (int j = 0; j < exact::kMaxLimbs; ++j) {
    if (j < k) {  // kernel-uniform
      for (int o = 32; o > 0; o >>= 1) a[j] += __shfl_xor(a[j], o);
      if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][j] = a[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < k) {
    long long sum = 0;
    for (int w = 0; w < kSqWaves; ++w) sum += s_part[w][threadIdx.x];
    if (sum)
      atomicAdd(reinterpret_cast<unsigned long long*>(cells + threadIdx.x), static_cast<unsigned long long>(sum));
  }
}

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" int dal_sq_error_format(const double* pred, const double* y, int64_t n, int32_t* low, int32_t* top,
                                   int32_t* dev_status, dal_stream_t stream) {
  if (!pred || !y || !low || !top || !dev_status) return DAL_ERR_ARG;
  if (n < 0 || n > INT32_MAX) return DAL_ERR_SHAPE;
  if (n == 0) return DAL_OK;
  hipLaunchKernelGGL(sq_error_format_kernel, dim3(static_cast<unsigned>(sq_blocks(n))), dim3(kSqThreads), 0,
                     as_stream(stream), pred, y, n, low, top, dev_status);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

extern "C" int dal_sq_error_accumulate(const double* pred, const double* y, int64_t n, int32_t q, int32_t k,
                                       int64_t* cells, dal_stream_t stream) {
  if (!pred || !y || !cells) return DAL_ERR_ARG;
  if (n < 0 || n > INT32_MAX) return DAL_ERR_SHAPE;
  if (k < 1 || k > DAL_RF_REG_MAX_LIMBS) return DAL_ERR_UNSUPPORTED;
  if (n == 0) return DAL_OK;
  hipLaunchKernelGGL(sq_error_accumulate_kernel, dim3(static_cast<unsigned>(sq_blocks(n))), dim3(kSqThreads), 0,
                     as_stream(stream), pred, y, n, static_cast<int>(q), static_cast<int>(k), cells);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}
