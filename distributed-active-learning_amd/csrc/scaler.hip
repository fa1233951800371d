// StandardScaler(withMean=True, withStd=True) on the GPU:
//   lal_direct_mllib_implementation/classes/dataset.py:163-173 (and :199-208,
//   :228-236, :257-271): every split is standardised by MLlib's scaler before
//   anything is trained or scored.
// MLlib's MultivariateOnlineSummarizer merges partition summaries in arrival
// order, and a float-atomic reduction would do the same: the last bit of mean
// or 1/std would depend on the order, and with it a forest split x <= t.  Here
// the column moments S1 = sum x and S2 = sum x*x are exact integers in limbs
// (scaler_exact.hpp over rf_exact_sum.hpp), added with 64-bit integer atomics:
// the same words for any row order, chunking or sharding.  mean and std are
// rounded once from the exact rationals on the host (dal.dataset).
//
//   format      per column: min lowest-set-bit exponent, max top-bit exponent
//               (int32 atomic min / max into the caller's arrays), and a
//               status bit for NaN / Inf.
//   accumulate  cells[d][K1 + K2] += limbs of x and of x*x.  A thread owns one
//               column over a strided set of rows and keeps its K1 + K2 int64
//               words in registers (no atomic in the row loop); the block's
//               row lanes are summed through LDS; one global atomic per
//               (block, column, word).
//   transform   z = (double(x) - mean) * factor in fp64, two roundings, no FMA;
//               +0.0 where factor == 0 (std == 0); written as fp32 or fp64.
//
// Thread mapping of all three: a block of 256 threads is (256 / CW) row lanes
// by CW columns, CW = the power of two >= min(d, 64): a wave reads up to 256
// contiguous bytes of a row, and d = 2 still fills every lane (128 row lanes).
// Column tiles of CW go to blockIdx.y.
#include <algorithm>
#include <climits>

#include "common.hpp"
#include "scaler_exact.hpp"

namespace dal {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxColTile = 64;
constexpr int kTargetBlocks = 2048;  // blocks of one launch: 8 per CU
constexpr int kUnroll = 4;           // rows a thread loads before it decodes them

struct Map {
  int cw_log2, col_tiles;
  int64_t rows_per_block;
};

Map make_map(int64_t n, int64_t d) {
  Map m{};
  while ((int64_t{1} << m.cw_log2) < std::min<int64_t>(d, kMaxColTile)) ++m.cw_log2;
  const int64_t cw = int64_t{1} << m.cw_log2, rl = kThreads / cw;
  m.col_tiles = static_cast<int>(ceil_div(d, cw));
  const int64_t blocks_x = std::max<int64_t>(1, kTargetBlocks / m.col_tiles);
  m.rows_per_block = rl * std::max<int64_t>(1, ceil_div(n, rl * blocks_x));
  return m;
}

__device__ __forceinline__ void add64(int64_t* p, int64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), static_cast<unsigned long long>(v));
}

__global__ __launch_bounds__(kThreads) void scaler_format_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                 int64_t ldx, int cw_log2, int64_t rows_per_block,
                                                                 int32_t* low, int32_t* top, int32_t* dev_status) {
  __shared__ int s_low[kThreads], s_top[kThreads];
  const int tid = threadIdx.x, cw = 1 << cw_log2, rl = kThreads >> cw_log2;
  const int c = blockIdx.y * cw + (tid & (cw - 1)), lane = tid >> cw_log2;
  int lo = scaler::kNoLow, hi = scaler::kNoTop, bad = 0;
  if (c < d) {
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_block;
    const int64_t r1 = min(n, r0 + rows_per_block);
    for (int64_t r = r0 + lane; r < r1; r += rl) {
      const uint32_t b = __float_as_uint(x[r * ldx + c]);
      if (!scaler::finite_f32(b)) {
        bad = 1;
        continue;
      }
      const exact::Parts p = scaler::parts_f32(b);
      if (!p.mant) continue;
      lo = min(lo, scaler::low_exponent(p));
      hi = max(hi, scaler::top_exponent(p));
    }
  }
  s_low[tid] = lo;
  s_top[tid] = hi;
  bad = __syncthreads_or(bad);
  if (tid == 0 && bad) atomicOr(dev_status, DAL_FLAG_NONFINITE);
  if (tid < cw && c < d) {  // lane 0 of each column: the block's row lanes
    for (int l = 1; l < rl; ++l) {
      lo = min(lo, s_low[l * cw + tid]);
      hi = max(hi, s_top[l * cw + tid]);
    }
    if (lo != scaler::kNoLow) atomicMin(&low[c], lo);
    if (hi != scaler::kNoTop) atomicMax(&top[c], hi);
  }
}

__global__ __launch_bounds__(kThreads) void scaler_accumulate_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                     int64_t ldx, const int32_t* __restrict__ q,
                                                                     int k1, int k2, int cw_log2,
                                                                     int64_t rows_per_block, int64_t* cells) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int64_t* s = reinterpret_cast<int64_t*>(smem);  // [k1 + k2][kThreads]
  const int tid = threadIdx.x, cw = 1 << cw_log2, rl = kThreads >> cw_log2;
  const int c = blockIdx.y * cw + (tid & (cw - 1)), lane = tid >> cw_log2;
  int64_t a1[exact::kMaxLimbs], a2[exact::kMaxLimbs];  // fixed indices: registers
#pragma unroll
  for (int j = 0; j < exact::kMaxLimbs; ++j) a1[j] = a2[j] = 0;
  if (c < d) {
    const int qc = q[c];
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_block;
    const int64_t r1 = min(n, r0 + rows_per_block);
    for (int64_t r = r0 + lane; r < r1; r += static_cast<int64_t>(kUnroll) * rl) {
      uint32_t b[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t rr = r + static_cast<int64_t>(u) * rl;
        b[u] = rr < r1 ? __float_as_uint(x[rr * ldx + c]) : 0u;  // +0.0 adds nothing
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const exact::Parts p = scaler::parts_f32(b[u]);
        const exact::Parts sq = scaler::square(p);
#pragma unroll
        for (int j = 0; j < exact::kMaxLimbs; ++j) {
          if (j < k1) a1[j] += exact::limb(p, qc, j);
          if (j < k2) a2[j] += exact::limb(sq, 2 * qc, j);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < exact::kMaxLimbs; ++j) {
    if (j < k1) s[j * kThreads + tid] = a1[j];
    if (j < k2) s[(k1 + j) * kThreads + tid] = a2[j];
  }
  __syncthreads();
  const int K = k1 + k2;
  for (int e = tid; e < (K << cw_log2); e += kThreads) {
    const int w = e >> cw_log2, cc = e & (cw - 1);
    const int col = blockIdx.y * cw + cc;
    if (col >= d) continue;
    int64_t sum = 0;
    for (int l = 0; l < rl; ++l) sum += s[w * kThreads + l * cw + cc];
    if (sum) add64(&cells[static_cast<int64_t>(col) * K + w], sum);
  }
}

template <class Out>
__global__ __launch_bounds__(kThreads) void scaler_transform_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                    int64_t ldx, const double* __restrict__ mean,
                                                                    const double* __restrict__ factor, int cw_log2,
                                                                    Out* __restrict__ out, int64_t ldo) {
  const int tid = threadIdx.x, cw = 1 << cw_log2, rl = kThreads >> cw_log2;
  const int c = blockIdx.y * cw + (tid & (cw - 1)), lane = tid >> cw_log2;
  if (c >= d) return;
  const double m = mean ? mean[c] : 0.0, f = factor ? factor[c] : 1.0;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * rl + lane; r < n; r += static_cast<int64_t>(gridDim.x) * rl) {
    double z = static_cast<double>(x[r * ldx + c]);
    if (mean) z = z - m;
    if (factor) z = f != 0.0 ? z * f : 0.0;
    out[r * ldo + c] = static_cast<Out>(z);
  }
}

int shape_check(int64_t n, int64_t d, int64_t ldx) {
  if (n < 0 || n > INT32_MAX || d < 1 || ldx < d) return DAL_ERR_SHAPE;
  if (ceil_div(d, kMaxColTile) > 65535) return DAL_ERR_SHAPE;
  return DAL_OK;
}

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" int64_t dal_scaler_rows_per_block(int64_t n, int64_t d) {
  if (n < 1 || d < 1) return 0;
  return make_map(n, d).rows_per_block;
}

extern "C" int dal_scaler_limbs(const int32_t* low, const int32_t* top, int64_t d, int32_t* k1, int32_t* k2,
                                int32_t* q, int64_t* bad_column) {
  if (!low || !top || !k1 || !k2) return DAL_ERR_ARG;
  if (d < 1) return DAL_ERR_SHAPE;
  const int64_t bad = scaler::limb_counts(low, top, d, k1, k2, q);
  if (bad_column) *bad_column = bad;
  return bad < 0 ? DAL_OK : DAL_ERR_UNSUPPORTED;
}

extern "C" int dal_scaler_format(const float* x, int64_t n, int64_t d, int64_t ldx, int32_t* low, int32_t* top,
                                 int32_t* dev_status, dal_stream_t stream) {
  if (!x || !low || !top || !dev_status) return DAL_ERR_ARG;
  if (const int rc = shape_check(n, d, ldx)) return rc;
  if (n == 0) return DAL_OK;
  const Map m = make_map(n, d);
  const dim3 grid(static_cast<unsigned>(ceil_div(n, m.rows_per_block)), static_cast<unsigned>(m.col_tiles));
  hipLaunchKernelGGL(scaler_format_kernel, grid, dim3(kThreads), 0, as_stream(stream), x, n, static_cast<int>(d),
                     ldx, m.cw_log2, m.rows_per_block, low, top, dev_status);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

extern "C" int dal_scaler_accumulate(const float* x, int64_t n, int64_t d, int64_t ldx, const int32_t* q,
                                     int32_t k1, int32_t k2, int64_t* cells, dal_stream_t stream) {
  if (!x || !q || !cells) return DAL_ERR_ARG;
  if (const int rc = shape_check(n, d, ldx)) return rc;
  if (k1 < 1 || k1 > DAL_RF_REG_MAX_LIMBS || k2 < 1 || k2 > DAL_RF_REG_MAX_LIMBS) return DAL_ERR_UNSUPPORTED;
  if (n == 0) return DAL_OK;
  const Map m = make_map(n, d);
  const dim3 grid(static_cast<unsigned>(ceil_div(n, m.rows_per_block)), static_cast<unsigned>(m.col_tiles));
  const size_t smem = static_cast<size_t>(k1 + k2) * kThreads * sizeof(int64_t);  // at most 32 KiB
  hipLaunchKernelGGL(scaler_accumulate_kernel, grid, dim3(kThreads), smem, as_stream(stream), x, n,
                     static_cast<int>(d), ldx, q, k1, k2, m.cw_log2, m.rows_per_block, cells);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

extern "C" int dal_scaler_transform(const float* x, int64_t n, int64_t d, int64_t ldx, const double* mean,
                                    const double* factor, void* out, int out_dtype, int64_t ldo,
                                    dal_stream_t stream) {
  if (!x || !out) return DAL_ERR_ARG;
  if (out_dtype != DAL_X_F32 && out_dtype != DAL_X_F64) return DAL_ERR_ARG;
  if (const int rc = shape_check(n, d, ldx)) return rc;
  if (ldo < d) return DAL_ERR_SHAPE;
  if (n == 0) return DAL_OK;
  const Map m = make_map(n, d);
  const int64_t rl = kThreads >> m.cw_log2;
  const int64_t blocks_x = std::max<int64_t>(1, kTargetBlocks / m.col_tiles);
  const dim3 grid(static_cast<unsigned>(std::min(ceil_div(n, rl), blocks_x)), static_cast<unsigned>(m.col_tiles));
  if (out_dtype == DAL_X_F64)
    hipLaunchKernelGGL(scaler_transform_kernel<double>, grid, dim3(kThreads), 0, as_stream(stream), x, n,
                       static_cast<int>(d), ldx, mean, factor, m.cw_log2, static_cast<double*>(out), ldo);
  else
    hipLaunchKernelGGL(scaler_transform_kernel<float>, grid, dim3(kThreads), 0, as_stream(stream), x, n,
                       static_cast<int>(d), ldx, mean, factor, m.cw_log2, static_cast<float*>(out), ldo);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}
