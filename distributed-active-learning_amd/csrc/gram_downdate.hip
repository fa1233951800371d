// Density downdate: growing the excluded set E by a batch Delta of m rows
// lowers every remaining density by sum_{j in Delta} <u_i, u_j> -- an N x m
// product over the split operand the pool already holds, not a new N^2 Gram.
//
// Reference: density_weighting.py:95-100 drops L0 from the proximity matrix
// once; the usual information density takes the sum over the CURRENT
// unlabeled pool, so rows leave it as they are labeled (dal.h,
// dal_density_downdate).
//
// Arithmetic.  The operand rows are H = fp16(2^12 u), L = fp16(2^12 u - H)
// (dal_split_f16's layout).  Per 32 features three v_mfma_f32_16x16x32_f16
// form H_i.H_j (one fp32 chain) and H_i.L_j + L_i.H_j (a second chain, 2^-11
// of the first in magnitude); L.L is not computed and is charged to the bound.
// The column index of a 16 x 16 result tile is a row of Delta, and only the
// sum over Delta is wanted, so every 16-row tile of Delta adds into the same
// accumulator tile.  Each accumulator ELEMENT is rounded on its own to a
// multiple of 2^-32 (the products are in units of 2^-24) after every
// kDeltaTile rows of Delta and kept as an int64 from there on: the 16 column
// lanes are added as integers at the end and one lane per row subtracts the
// total from acc.  No step depends on the grid, so acc's bytes do not either.
//
// Shape.  A block is 4 waves; a wave keeps the A fragments (H and L) of 32
// pool rows over a chunk of <= 256 features in registers (128 VGPRs at 256)
// and sweeps Delta in LDS tiles of kDeltaTile = 64 rows (64 KB at 256
// features; 16-byte slots XOR-swizzled by row, so the B-fragment ds_read_b128
// of 16 rows at one feature offset spread over the banks).  Two blocks per CU
// hide one block's tile fill under the other's MFMAs.  The pool operand is
// read from HBM once; Delta (<= 1 MB) is re-read from L2 by every block.
#include "common.hpp"

namespace dal {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kDeltaTile = DAL_DOWNDATE_TILE;  // rows of Delta per LDS tile and per fold
constexpr int kRowTiles = 2;                   // 16-row tiles of the pool per wave
constexpr int kWaves = 4;
constexpr int kBlockRows = kWaves * kRowTiles * 16;  // 128: divides n_pad (a multiple of 256)
static_assert(kDeltaTile % 16 == 0 && 256 % kBlockRows == 0, "whole tiles");

int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 256;
  return cus;
}

// CHUNK features of a row are 2 * CHUNK contiguous halves of the operand
// (whole [KS H | KS L] slices), at half offset c * 2 * CHUNK for chunk c.
// Feature f of the chunk: H at (f / KS) * 2 * KS + f % KS, L at + KS.
template <int CHUNK, int KS>
__global__ __launch_bounds__(kWaves * 64, 2) void density_downdate_kernel(
    const uint16_t* __restrict__ ops, int64_t n_pad, int64_t d_pad, const uint16_t* __restrict__ delta,
    int m_tiles, long long* __restrict__ acc) {
  constexpr int kSteps = CHUNK / 32;             // MFMA k-steps per chunk
  constexpr int kSlots = 2 * CHUNK / 8;          // 16-byte slots per row of the chunk
  constexpr int kSwz = kSlots - 1 < 15 ? kSlots - 1 : 15;
  __shared__ uint4 tile[kDeltaTile * kSlots];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int64_t row_halves = 2 * d_pad;
  const int n_chunks = static_cast<int>(d_pad / CHUNK);
  const int64_t n_groups = n_pad / kBlockRows;

  for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int64_t wrow0 = g * kBlockRows + wave * (kRowTiles * 16);
    long long fix[kRowTiles][4];
#pragma unroll
    for (int t = 0; t < kRowTiles; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) fix[t][i] = 0;

    for (int c = 0; c < n_chunks; ++c) {
      // this wave's A fragments: lane holds row lr of each tile, features 32 s + 8 lq .. + 7
      f16x8 ah[kRowTiles][kSteps], al[kRowTiles][kSteps];
#pragma unroll
      for (int t = 0; t < kRowTiles; ++t) {
        const uint16_t* rp = ops + (wrow0 + t * 16 + lr) * row_halves + static_cast<int64_t>(c) * 2 * CHUNK;
#pragma unroll
        for (int s = 0; s < kSteps; ++s) {
          const int f0 = 32 * s;
          const int h = (f0 / KS) * 2 * KS + f0 % KS + 8 * lq;
          ah[t][s] = *reinterpret_cast<const f16x8*>(rp + h);
          al[t][s] = *reinterpret_cast<const f16x8*>(rp + h + KS);
        }
      }
      for (int dt = 0; dt < m_tiles; ++dt) {
        __syncthreads();  // the previous tile's readers are done
        for (int e = tid; e < kDeltaTile * kSlots; e += kWaves * 64) {
          const int r = e / kSlots, sl = e % kSlots;
          const uint16_t* sp = delta + (static_cast<int64_t>(dt) * kDeltaTile + r) * row_halves +
                               static_cast<int64_t>(c) * 2 * CHUNK + sl * 8;
          tile[r * kSlots + (sl ^ (r & kSwz))] = *reinterpret_cast<const uint4*>(sp);
        }
        __syncthreads();
        f32x4 ch[kRowTiles], cx[kRowTiles];
#pragma unroll
        for (int t = 0; t < kRowTiles; ++t) {
          ch[t] = f32x4{0.f, 0.f, 0.f, 0.f};
          cx[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int bt = 0; bt < kDeltaTile / 16; ++bt) {
          const int r = bt * 16 + lr;  // the Delta row this lane's B fragment holds
#pragma unroll
          for (int s = 0; s < kSteps; ++s) {
            const int f0 = 32 * s;
            const int slot = ((f0 / KS) * 2 * KS + f0 % KS) / 8 + lq;
            const uint4 qh = tile[r * kSlots + (slot ^ (r & kSwz))];
            const uint4 ql = tile[r * kSlots + ((slot + KS / 8) ^ (r & kSwz))];
            const f16x8 bh = __builtin_bit_cast(f16x8, qh);
            const f16x8 bl = __builtin_bit_cast(f16x8, ql);
#pragma unroll
            for (int t = 0; t < kRowTiles; ++t) {
              ch[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t][s], bh, ch[t], 0, 0, 0);
              cx[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t][s], bl, cx[t], 0, 0, 0);
              cx[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[t][s], bh, cx[t], 0, 0, 0);
            }
          }
        }
        // fold: every element on its own to a multiple of 2^-32 (2^-24 units x 2^8)
#pragma unroll
        for (int t = 0; t < kRowTiles; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            fix[t][i] += static_cast<long long>(__builtin_rint(static_cast<double>(ch[t][i]) * 256.0));
            fix[t][i] += static_cast<long long>(__builtin_rint(static_cast<double>(cx[t][i]) * 256.0));
          }
      }
    }
    // integer sum over the 16 column lanes; lane lr == 0 owns rows 4 lq .. 4 lq + 3 of each tile
#pragma unroll
    for (int t = 0; t < kRowTiles; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        long long v = fix[t][i];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
        if (lr == 0) {
          const int64_t row = wrow0 + t * 16 + lq * 4 + i;
          acc[row] = acc[row] - v;
        }
      }
  }
}

template <int CHUNK, int KS>
int launch(const uint16_t* ops, int64_t n_pad, int64_t d_pad, const uint16_t* delta, int64_t m, long long* acc,
           int grid_blocks, hipStream_t st) {
  const int64_t groups = n_pad / kBlockRows;
  int64_t grid = grid_blocks > 0 ? grid_blocks : 2 * static_cast<int64_t>(device_cus());
  if (grid > groups) grid = groups;
  const int m_tiles = static_cast<int>(ceil_div(m, kDeltaTile));
  hipLaunchKernelGGL((density_downdate_kernel<CHUNK, KS>), dim3(static_cast<unsigned>(grid)), dim3(kWaves * 64), 0, st,
                     ops, n_pad, d_pad, delta, m_tiles, acc);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

// Features per register-resident chunk of the kernel that runs d_pad.
int downdate_chunk(int64_t d_pad) { return d_pad >= 256 ? 256 : static_cast<int>(d_pad); }

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" double dal_density_downdate_error_bound(int64_t m, int64_t d_pad) {
  // |applied decrement - canonical sum_{j in Delta} <u_i, u_j>| per row, the
  // model of dal_density_error_bound_sym_d: u = 2^-23 for the MFMA's internal
  // fp32 adds (counted as sequential adds), products exact (f16 x f16), c = 1
  // + 2^-8 >= sum_f |h_i h_j| / 2^24 (Cauchy-Schwarz on unit rows).  Per row
  // of Delta:
  //   H.H chain     (kDeltaTile / 16) tiles x chunk features between two folds
  //                 (1,024 products at d_pad >= 256):            gamma_chain * c
  //   H.L + L.H     twice as many products, each |l| <= 2^-11 |h|:
  //                                                   gamma_(2 chain) * 2^-10 * c
  //   L.L dropped   sum_f |l_i l_j| <= 2^-22 sum_f |h_i h_j|:          2^-22 * c
  //   split + fp32 unit rows (as the cold bound)                        5 * 2^-22
  // and per fold (ceil(m / kDeltaTile) x d_pad / chunk of them) 32 element
  // roundings to 2^-32 (16 columns, two chains): 32 * 2^-33.
  if (m < 1) m = 1;
  const double u = 1.0 / 8388608.0;  // 2^-23
  auto gamma = [u](double n) { return n * u / (1.0 - n * u); };
  const double s = 1.0 / 4194304.0;  // 2^-22
  const double c = 1.0 + 1.0 / 256.0;
  const int chunk = d_pad > 0 ? downdate_chunk(d_pad) : 256;
  const double chain = static_cast<double>(kDeltaTile / 16) * chunk;
  const double per_col = gamma(chain) * c + gamma(2.0 * chain) * c / 1024.0 + s * c + 5.0 * s + 1e-10;
  const double folds =
      static_cast<double>(ceil_div(m, kDeltaTile)) * static_cast<double>(d_pad > 0 ? ceil_div(d_pad, chunk) : 1);
  return per_col * static_cast<double>(m) + folds * 32.0 / 8589934592.0 + 1e-9;
}

extern "C" int dal_density_downdate(const uint16_t* ops, int64_t n_pad, int64_t d_pad, const uint16_t* delta_ops,
                                    int64_t m, int64_t* acc, int grid_blocks, dal_stream_t stream) {
  if (!ops || !delta_ops || !acc) return DAL_ERR_ARG;
  if (n_pad < 256 || n_pad % 256) return DAL_ERR_SHAPE;
  if (d_pad < 1 || d_pad != dal_pad_features(d_pad)) return DAL_ERR_SHAPE;
  if (m < 1) return DAL_ERR_SHAPE;
  if (m > DAL_DOWNDATE_MAX_ROWS) return DAL_ERR_CAPACITY;
  if ((reinterpret_cast<uintptr_t>(ops) | reinterpret_cast<uintptr_t>(delta_ops)) & 15) return DAL_ERR_ARG;
  hipStream_t st = as_stream(stream);
  long long* a = reinterpret_cast<long long*>(acc);
  switch (downdate_chunk(d_pad)) {
    case 32:
      return launch<32, 32>(ops, n_pad, d_pad, delta_ops, m, a, grid_blocks, st);
    case 64:
      return launch<64, 64>(ops, n_pad, d_pad, delta_ops, m, a, grid_blocks, st);
    case 128:
      return launch<128, 128>(ops, n_pad, d_pad, delta_ops, m, a, grid_blocks, st);
    default:
      return launch<256, 128>(ops, n_pad, d_pad, delta_ops, m, a, grid_blocks, st);
  }
}
