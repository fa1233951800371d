// The fp4 form's whole preparation in one pass over the pool (dal_prep_split_fp4):
// what dal_prep_split (norms, split operand, canonical column-sum partials,
// zeroed accumulator), dal_quant_fp4 (e2m1 codes) and launch 1 of
// dal_gram_sym_residual_fp4 (sigma^H' per super block, S^L') produce, the same
// bytes, from one fp64 quotient and one a4 per element.
//
// A block walks whole 512-row super blocks, two canonical 256-row chunks each:
//  1. norms: thread t owns row t of the chunk; the row reaches it through an LDS
//     tile, 32 features at a time (coalesced loads), and is summed in the
//     canonical sequential fp64 order -- every thread has a row;
//  2. elements: thread t owns feature t of a 256-feature slice and walks the
//     chunk's rows in order (the second read of the chunk, from cache): q =
//     double(x) / norm is the column-sum term AND, rounded to fp32, the unit
//     row's element; its split (H, L), a4(H), the code, h' and l' follow in
//     registers.  The column partial is the thread's own sequential chain;
//     sigma^H' and the block's share of S^L' are the thread's own exact sums --
//     no reduction anywhere.  H, L and the codes of 8 rows are staged in LDS in
//     the operand's layout and leave in 16-byte stores.
// S^L': one partial per block and feature (a block adds its super blocks'
// sums into its own words), totalled by a small second launch -- no atomics on
// the pool-wide d_pad addresses (the comment above csym_sigma_kernel).

#include "common.hpp"
#include "gram_fp4.hpp"

namespace dal {
namespace {

constexpr int kPfRows = DAL_CANON_CHUNK;  // rows per chunk = threads per block
constexpr int kPfSB = 512;                // super block rows (gram_sym.hip kSB)
// tuning constants (A/B builds: scripts/ab_build.sh; profiles/r16/prep_fused)
#ifndef DAL_PREP_TILE
#define DAL_PREP_TILE 32   // features per norm tile
#endif
#ifndef DAL_PREP_BATCH
#define DAL_PREP_BATCH 8   // rows staged per store round (16: the divisions spill at 128 registers)
#endif
#ifndef DAL_PREP_WAVES
#define DAL_PREP_WAVES 4   // waves per SIMD = blocks per CU (128 registers; the LDS admits four as well)
#endif
constexpr int kPfTile = DAL_PREP_TILE;
constexpr int kPfBatch = DAL_PREP_BATCH;
constexpr int kPfWaves = DAL_PREP_WAVES;
static_assert(kPfTile % 16 == 0 && 256 % kPfTile == 0 && kPfBatch % 4 == 0 && 256 % kPfBatch == 0, "tile and batch");
constexpr int kPfMaxBlocks = 4096;        // S^L' partial rows at most
static_assert(kPfRows == 256 && kPfSB == 2 * kPfRows, "a super block is two canonical chunks");

constexpr int kPfLive = 1;   // in the pool and not excluded: a column-sum term
constexpr int kPfUnit = 2;   // ... and a positive norm: a unit row

__global__ __launch_bounds__(kPfRows) __attribute__((amdgpu_waves_per_eu(kPfWaves, kPfWaves))) void prep_split_fp4_kernel(
    const float* __restrict__ x, int64_t n, int d, int64_t ldx, const uint8_t* __restrict__ flags, int d_pad,
    int nsb, int qg, uint16_t* __restrict__ out, double* __restrict__ norm64, int32_t* __restrict__ status,
    long long* __restrict__ acc_zero, double* __restrict__ partials, uint8_t* __restrict__ codes,
    long long* __restrict__ sig_h, long long* __restrict__ sl_parts) {
  // the norm tile and the store stage are never live together
  constexpr int kTileBytes = kPfRows * (kPfTile + 1) * 4;
  constexpr int kStageBytes = kPfBatch * 1024 + kPfBatch * 256;  // [rows][H 128 | L 128 | H 128 | L 128] + [rows][256] codes
  __shared__ __attribute__((aligned(16))) unsigned char smem[kTileBytes > kStageBytes ? kTileBytes : kStageBytes];
  __shared__ double rnorm[kPfRows];
  __shared__ uint8_t rlive[kPfRows];
  float(*tile)[kPfTile + 1] = reinterpret_cast<float(*)[kPfTile + 1]>(smem);
  uint16_t* stage = reinterpret_cast<uint16_t*>(smem);
  uint8_t* cstage = smem + kPfBatch * 1024;
  const int tid = threadIdx.x;
  const int n_slices = d_pad / 256;
  const int q_begin = static_cast<int>(blockIdx.x) * qg;
  const int q_end = q_begin + qg < nsb ? q_begin + qg : nsb;
  // position of feature tid's H term in a row's 512 staged halves
  const int spos = (tid >> 7) * 256 + (tid & 127);
  for (int Q = q_begin; Q < q_end; ++Q) {
    for (int half = 0; half < 2; ++half) {
      const int64_t c = 2 * static_cast<int64_t>(Q) + half;
      const int64_t row0 = c * kPfRows;
      // ---- 1. norms of the chunk ----
      __syncthreads();  // the previous chunk's last stage is stored
      {
        double n2 = 0.0;
        if (row0 < n) {
          for (int c0 = 0; c0 < d; c0 += kPfTile) {
            if (c0) __syncthreads();  // the previous tile is summed
            // rounds of 16 independent loads (rows r, r + 256 / kPfTile, ...)
            const int r_t = tid / kPfTile, cc = tid % kPfTile;
            const bool cf = c0 + cc < d;
            const float* xt = x + (row0 + r_t) * ldx + c0 + cc;
            constexpr int kStep = kPfRows / kPfTile;  // rows between a thread's loads
#pragma unroll 1
            for (int j0 = 0; j0 < kPfTile; j0 += 16) {
              float v[16];
#pragma unroll
              for (int j = 0; j < 16; ++j) {
                const int r = r_t + kStep * (j0 + j);
                v[j] = (cf && row0 + r < n) ? xt[static_cast<int64_t>(kStep * (j0 + j)) * ldx] : 0.0f;
              }
#pragma unroll
              for (int j = 0; j < 16; ++j) tile[r_t + kStep * (j0 + j)][cc] = v[j];
            }
            __syncthreads();
            const int cmax = d - c0 < kPfTile ? d - c0 : kPfTile;
            if (cmax == kPfTile) {
#pragma unroll
              for (int cc = 0; cc < kPfTile; ++cc) {
                const double w = static_cast<double>(tile[tid][cc]);
                n2 = n2 + w * w;  // -ffp-contract=off: mul then add (canonical order)
              }
            } else {
              for (int cc = 0; cc < cmax; ++cc) {
                const double w = static_cast<double>(tile[tid][cc]);
                n2 = n2 + w * w;
              }
            }
          }
        }
        const int64_t row = row0 + tid;
        const double nr = __builtin_sqrt(n2);
        int live = 0;
        if (row < n) {
          if (!(n2 > 0.0)) atomicOr(status, DAL_FLAG_ZERO_NORM);
          norm64[row] = nr;
          if (!(flags && (flags[row] & DAL_ROW_EXCLUDED))) live = kPfLive | (nr > 0.0 ? kPfUnit : 0);
        }
        if (acc_zero) acc_zero[row] = 0;  // (row < n_pad: whole super blocks)
        rnorm[tid] = nr;
        rlive[tid] = static_cast<uint8_t>(live);
      }
      // ---- 2. the chunk's rows in order, feature f of each slice ----
      for (int s = 0; s < n_slices; ++s) {
        const int f = s * 256 + tid;
        const bool lf = f < d;
        int sum_g = 0;       // sum of a4 over the chunk's rows (|.| <= 256 * 12)
        double sum_l = 0.0;  // sum of l' (exact: multiples of 2^-24 below 2^13, 256 terms)
        double colacc = 0.0;
        float xv[kPfBatch];
#pragma unroll
        for (int j = 0; j < kPfBatch; ++j) xv[j] = (lf && row0 + j < n) ? x[(row0 + j) * ldx + f] : 0.0f;
        for (int rb = 0; rb < kPfRows; rb += kPfBatch) {
          float xn[kPfBatch];  // the next batch, in flight under this one's divisions
#pragma unroll
          for (int j = 0; j < kPfBatch; ++j) {
            const int64_t row = row0 + rb + kPfBatch + j;
            xn[j] = (lf && rb + kPfBatch < kPfRows && row < n) ? x[row * ldx + f] : 0.0f;
          }
          __syncthreads();  // the norms are written / the previous batch's stage is stored
#pragma unroll
          for (int j = 0; j < kPfBatch; ++j) {
            const int r = rb + j;
            const int live = rlive[r];  // (uniform over the block)
            float v = 0.0f;
            if (live & kPfLive) {
              // Excluded / padding rows contribute +0.0: the running sum starts at
              // +0.0 and can never become -0.0, so skipping them is bit-identical.
              const double q = static_cast<double>(xv[j]) / rnorm[r];
              colacc = colacc + q;
              if ((live & kPfUnit) && lf) v = static_cast<float>(q);
            }
            const float sv = v * 4096.0f;  // exact
            const _Float16 he = static_cast<_Float16>(sv);
            const _Float16 le = static_cast<_Float16>(sv - static_cast<float>(he));
            const float hf = static_cast<float>(he);
            const int g = quant_fp4(hf);
            // l' = (h - h') + l as requant_fp4 forms it
            double hd = static_cast<double>(hf), ld = static_cast<double>(static_cast<float>(le));
            requant_fp4(hd, ld);
            sum_g += g;
            sum_l += ld;
            stage[j * 512 + spos] = __builtin_bit_cast(uint16_t, he);
            stage[j * 512 + spos + 128] = __builtin_bit_cast(uint16_t, le);
            cstage[j * 256 + tid] = static_cast<uint8_t>(code_fp4(g));
          }
          __syncthreads();
          // H | L: 64 16-byte chunks per row and slice, contiguous in the operand
#pragma unroll
          for (int k = 0; k < kPfBatch * 64 / kPfRows; ++k) {
            const int idx = tid + kPfRows * k, j = idx >> 6, cc = idx & 63;
            const int64_t row = row0 + rb + j;
            reinterpret_cast<uint4*>(out + row * (2 * static_cast<int64_t>(d_pad)) + s * 512)[cc] =
                reinterpret_cast<const uint4*>(stage)[idx];
          }
          // codes: 8 16-byte chunks per row and slice, 32 staged bytes each
          if (tid < kPfBatch * 8) {
            const int j = tid >> 3, cc = tid & 7;
            const uint4* src = reinterpret_cast<const uint4*>(cstage + j * 256 + cc * 32);
            const uint4 a = src[0], b = src[1];
            const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              uint32_t p = 0;
#pragma unroll
              for (int h2 = 0; h2 < 2; ++h2) {
                const uint32_t u = w[2 * k + h2];  // four code bytes -> four nibbles
                const uint32_t nib = (u & 0xFu) | ((u >> 4) & 0xF0u) | ((u >> 8) & 0xF00u) | ((u >> 12) & 0xF000u);
                p |= nib << (16 * h2);
              }
              o[k] = p;
            }
            const int64_t row = row0 + rb + j;
            reinterpret_cast<uint4*>(codes + row * (d_pad / 2) + s * 128)[cc] = uint4{o[0], o[1], o[2], o[3]};
          }
#pragma unroll
          for (int j = 0; j < kPfBatch; ++j) xv[j] = xn[j];
        }
        if (partials && lf && row0 < n) partials[c * d + f] = colacc;
        // sigma^H' of the super block and the block's share of S^L', units of
        // 2^-24: this thread's own words, the second chunk adds to the first's
        long long* sg = sig_h + static_cast<int64_t>(Q) * d_pad + f;
        const long long gq = static_cast<long long>(sum_g) * (1LL << 29);  // h' = 32 a4, times 2^24
        *sg = half == 0 ? gq : *sg + gq;
        long long* slp = sl_parts + static_cast<int64_t>(blockIdx.x) * d_pad + f;
        const long long lq = static_cast<long long>(sum_l * 16777216.0);
        *slp = (Q == q_begin && half == 0) ? lq : *slp + lq;
      }
    }
  }
}

// S^L'[f] = the sum of the blocks' partials; wave w of the block takes the
// partial rows w, w + 16, ... (one dependent load after another: 26 us for 977 rows)
__global__ __launch_bounds__(1024) void prep_sl_total_kernel(const long long* __restrict__ parts, int n_parts,
                                                             int d_pad, long long* __restrict__ s_l) {
  __shared__ long long red[16][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int f = blockIdx.x * 64 + lane;
  long long v = 0;
  if (f < d_pad) {
    for (int p0 = w; p0 < n_parts; p0 += 16 * 8) {  // 8 loads in flight
      long long t[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        t[j] = p0 + 16 * j < n_parts ? parts[static_cast<int64_t>(p0 + 16 * j) * d_pad + f] : 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) v += t[j];
    }
  }
  red[w][lane] = v;
  __syncthreads();
  if (w == 0 && f < d_pad) {
    long long t = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][lane];
    s_l[f] = t;
  }
}

int prep_blocks(int64_t nsb, int* qg_out) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  // super blocks per block: one round of resident blocks
  int64_t qg = ceil_div(nsb, kPfWaves * static_cast<int64_t>(cus));
  if (qg < ceil_div(nsb, kPfMaxBlocks)) qg = ceil_div(nsb, kPfMaxBlocks);
  if (qg < 1) qg = 1;
  *qg_out = static_cast<int>(qg);
  return static_cast<int>(ceil_div(nsb, qg));
}

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" size_t dal_prep_split_fp4_workspace_bytes(int64_t n_pad, int64_t d_pad) {
  if (n_pad <= 0 || d_pad <= 0) return 0;
  const int64_t nsb = n_pad / kPfSB;
  return static_cast<size_t>(nsb < kPfMaxBlocks ? nsb : kPfMaxBlocks) * static_cast<size_t>(d_pad) * 8;
}

extern "C" int dal_prep_split_fp4(const float* x, int64_t n, int64_t d, int64_t x_stride, const uint8_t* row_flags,
                                  int64_t n_pad, int64_t d_pad, uint16_t* out, double* norm64, double* partials,
                                  int64_t* acc_zero, uint8_t* out_fp4, int64_t* sigma_h, int64_t* s_l, void* ws,
                                  size_t ws_bytes, int32_t* dev_status, dal_stream_t stream) {
  if (!x || !out || !norm64 || !out_fp4 || !sigma_h || !s_l || !ws || !dev_status) return DAL_ERR_ARG;
  const int64_t ldx = x_stride;
  if (n < 1 || d < 1 || ldx < d || n_pad < n || n_pad % DAL_ROW_GRANULE || n_pad % kPfSB || d > (1 << 20))
    return DAL_ERR_SHAPE;
  if (d_pad != dal_pad_features(d_pad) || d_pad < d || d_pad % 256) return DAL_ERR_SHAPE;
  if (n_pad / kPfSB > INT32_MAX / 2) return DAL_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(out_fp4)) & 15) return DAL_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(sigma_h) | reinterpret_cast<uintptr_t>(s_l)) & 7)
    return DAL_ERR_SHAPE;
  if (ws_bytes < dal_prep_split_fp4_workspace_bytes(n_pad, d_pad)) return DAL_ERR_SHAPE;
  const int64_t nsb = n_pad / kPfSB;
  int qg = 1;
  const int blocks = prep_blocks(nsb, &qg);
  hipStream_t st = as_stream(stream);
  long long* parts = static_cast<long long*>(ws);
  hipLaunchKernelGGL(prep_split_fp4_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kPfRows), 0, st, x, n,
                     static_cast<int>(d), ldx, row_flags, static_cast<int>(d_pad), static_cast<int>(nsb), qg, out,
                     norm64, dev_status, reinterpret_cast<long long*>(acc_zero), partials, out_fp4,
                     reinterpret_cast<long long*>(sigma_h), parts);
  DAL_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(prep_sl_total_kernel, dim3(static_cast<unsigned>(ceil_div(d_pad, 64))), dim3(1024), 0, st, parts,
                     blocks, static_cast<int>(d_pad), reinterpret_cast<long long*>(s_l));
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}
