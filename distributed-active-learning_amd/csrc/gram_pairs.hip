// Thresholded cosine pairs: every pair i < j of pool rows whose canonical fp64
// cosine reaches a threshold tau, exactly, with the N x N matrix never stored.
//
// Reference: final_thesis/similarity.py:34-38 (columnSimilarities of the
// normalised pool; MLlib's own columnSimilarities(threshold) is the sampled
// DIMSUM form of the same question).
//
// Two kernels, in the style of the selection paths: a cheap MFMA filter with a
// rigorous error bound, then the few candidates inside the bound re-decided in
// canonical fp64.
//
// Filter (pairs_filter_kernel).  A symmetric GEMM over the block pairs P <= Q
// (256-row blocks) of the H runs of the split operand (dal_prep_split: H =
// fp16(2^12 u), layout [n_pad][d_pad / KS][KS H | KS L]; the L runs are not
// read).  The whole dot product over d_pad sits in one accumulator before it
// is compared, so the output tile is register resident and the loop runs over
// K: a block of 4 waves owns one 128 x 128 tile (pairs_schedule.hpp maps the
// linear block index to (P, Q, sub tile)), each wave 64 x 64 of it as 4 x 4
// v_mfma_f32_16x16x32_f16 accumulators (64 VGPRs).  H is staged through LDS BK
// features at a time (BK = 64, or 32 at d_pad 32): global -> registers -> LDS,
// two LDS buffers, the next stage's global loads in flight while the current
// one is multiplied, one barrier per stage.  LDS rows are BK halves; the 16-B
// chunk c of row r sits at c ^ swz(r) (the swizzles of gram_sym.hip's stages:
// conflict-free ds_read_b128 for the MFMA fragment pattern).
//
// Epilogue.  acc is <H_i, H_j> in units of 2^-24.  A lane keeps an entry when
// acc >= (tau - bound) * 2^24 (compared in fp32 against a threshold rounded
// towards -inf: the filter can only over-admit), i < j (global rows), j < n,
// and neither row is DAL_ROW_EXCLUDED.  The common case -- no accumulator of
// the wave reaches the threshold -- is one compare per accumulator and a
// ballot.  Otherwise the wave counts its hits, reserves slots with one global
// atomic, and writes (i << 32 | j, acc * 2^-24) per candidate below cap; the
// counter keeps counting past cap, nothing is written beyond it, and the
// overflow sets DAL_FLAG_CAND_OVERFLOW.
//
// Resolve (pairs_resolve_kernel).  One thread per candidate: u = x / norm64 per
// element in fp64, sum_f u_if * u_jf over the d real features, ascending f,
// multiply then add, no FMA -- the oracle's max_cosine_canonical definition,
// symmetric in (i, j) bit for bit.
#include <math.h>
#include <stdlib.h>

#include "common.hpp"
#include "pairs_schedule.hpp"

namespace dal {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kPairThreads = 256;  // 4 waves, 2 x 2 over the 128 x 128 tile

template <int BK>
struct PairCfg {
  static constexpr int CH = BK / 8;                         // 16-B chunks per staged row
  static constexpr int NL = kPairTile * CH / kPairThreads;  // chunks per thread per operand per stage
  static constexpr int NKS = BK / 32;                       // MFMA k-steps per stage
  static constexpr int OPER = kPairTile * CH;               // chunks per operand per stage
  static constexpr int OCC = 2;  // blocks per CU (BK 64: 64 KiB of LDS each; 3 or 4 at BK 32 spill)
  // chunk position XOR of a staged row (see gram_sym.hip, Cfg::swz)
  static __host__ __device__ constexpr int swz(int row) {
    return CH >= 8 ? row & (CH - 1) : ((row >> 2) & 3) ^ (((row >> 2) & 1) << 1);
  }
  static_assert(CH == 4 || CH == 8, "swizzles for 4 and 8 chunks per row");
  static_assert(NL >= 1 && NL * kPairThreads == OPER, "the threads cover a stage exactly");
};

template <int BK>
__global__ __launch_bounds__(kPairThreads, (PairCfg<BK>::OCC)) void pairs_filter_kernel(
    const uint16_t* __restrict__ rows, int64_t row_block0, int64_t n_row_blocks, const uint16_t* __restrict__ cols,
    int64_t col_block0, int64_t j_lo, int64_t j_hi, int64_t n_total, int d_pad, int ks,
    const uint8_t* __restrict__ row_flags, float thr_scaled, int64_t cap, unsigned long long* __restrict__ keys,
    float* __restrict__ approx, unsigned long long* __restrict__ count, int32_t* __restrict__ dev_status) {
  using C = PairCfg<BK>;
  __shared__ uint4 lds[2][2][C::OPER];  // [buffer][A | B][row * CH + chunk position]

  const PairSchedule sched(row_block0, n_row_blocks, j_lo, j_hi);
  // (a 2-D grid: one dimension of 256-thread blocks ends at 2^32 threads, 16.7M tiles)
  const int64_t tile = static_cast<int64_t>(blockIdx.y) * gridDim.x + blockIdx.x;
  if (tile >= sched.tiles()) return;
  const int sub = static_cast<int>(tile % kPairSubTiles);
  const BlockPair bp = sched.pair(tile / kPairSubTiles);
  const int64_t P = bp.P, Q = bp.Q;
  if (!PairSchedule::sub_live(P, Q, sub)) return;  // (block-uniform)
  const int64_t i0 = P * kPairBlock + PairSchedule::sub_row(sub) * kPairTile;  // global first row / column
  const int64_t j0 = Q * kPairBlock + PairSchedule::sub_col(sub) * kPairTile;
  if (i0 >= n_total || j0 >= n_total) return;  // padding rows only

  const int64_t ldh = 2 * static_cast<int64_t>(d_pad);
  const uint16_t* arow = rows + (i0 - row_block0 * kPairBlock) * ldh;
  const uint16_t* brow = cols + (j0 - col_block0 * kPairBlock) * ldh;

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, lq = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;

  // stage loads: chunk e = tid + 256 j is chunk e % CH of tile row e / CH
  // (macros, not lambdas: the staging registers must not be addressable)
  uint4 ra[C::NL], rb[C::NL];
#define DAL_PAIRS_GLOAD(F0)                                                                     \
  do {                                                                                          \
    const int f0_ = (F0);                                                                       \
    const int64_t hoff_ = static_cast<int64_t>(f0_ / ks) * 2 * ks + f0_ % ks; /* the H run */  \
    _Pragma("unroll") for (int j = 0; j < C::NL; ++j) {                                         \
      const int e = tid + kPairThreads * j, r = e / C::CH, c = e % C::CH;                       \
      ra[j] = *reinterpret_cast<const uint4*>(arow + r * ldh + hoff_ + c * 8);                  \
      rb[j] = *reinterpret_cast<const uint4*>(brow + r * ldh + hoff_ + c * 8);                  \
    }                                                                                           \
  } while (0)
#define DAL_PAIRS_LSTORE(BUF)                                                                   \
  do {                                                                                          \
    _Pragma("unroll") for (int j = 0; j < C::NL; ++j) {                                         \
      const int e = tid + kPairThreads * j, r = e / C::CH, c = e % C::CH;                       \
      lds[BUF][0][r * C::CH + (c ^ C::swz(r))] = ra[j];                                         \
      lds[BUF][1][r * C::CH + (c ^ C::swz(r))] = rb[j];                                         \
    }                                                                                           \
  } while (0)

  f32x4 acc[4][4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment of tile row (base + t * 16 + li), features c * 32 + lq * 8 ..: the
  // tiles start at multiples of 16 rows, so swz(row) = swz(li)
  const int sw = C::swz(li);
  auto compute = [&](int buf) {
#pragma unroll
    for (int c = 0; c < C::NKS; ++c) {
      f16x8 a[4], b[4];
      const int pos = (c * 4 + lq) ^ sw;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a[t] = __builtin_bit_cast(f16x8, lds[buf][0][(wr * 64 + t * 16 + li) * C::CH + pos]);
        b[t] = __builtin_bit_cast(f16x8, lds[buf][1][(wc * 64 + t * 16 + li) * C::CH + pos]);
      }
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[rt], b[ct], acc[rt][ct], 0, 0, 0);
    }
  };

  // stage s is multiplied from buffer s & 1 while stage s + 1 travels global
  // -> registers; it is written to the other buffer (last read in stage s - 1,
  // behind the barrier that ended that stage) once the MFMAs are issued
  const int n_stages = d_pad / BK;
  DAL_PAIRS_GLOAD(0);
  DAL_PAIRS_LSTORE(0);
  __syncthreads();
  for (int s = 0; s + 1 < n_stages; ++s) {
    DAL_PAIRS_GLOAD((s + 1) * BK);
    compute(s & 1);
    DAL_PAIRS_LSTORE((s & 1) ^ 1);
    __syncthreads();
  }
  compute((n_stages - 1) & 1);
#undef DAL_PAIRS_GLOAD
#undef DAL_PAIRS_LSTORE

  // ---- epilogue: acc[rt][ct][q] is row ib + rt * 16 + lq * 4 + q, column jb + ct * 16 + li
  bool any = false;
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int q = 0; q < 4; ++q) any |= acc[rt][ct][q] >= thr_scaled;
  if (__builtin_amdgcn_ballot_w64(any) == 0) return;  // (wave-uniform; no barrier follows)

  const int64_t ib = i0 + wr * 64 + lq * 4;
  const int64_t jb = j0 + wc * 64 + li;
  // excluded rows / columns of this lane, one bit per (rt, q) and per ct
  unsigned ex_i = 0, ex_j = 0;
  if (row_flags) {
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t i = ib + rt * 16 + q;
        if (i < n_total && (row_flags[i] & DAL_ROW_EXCLUDED)) ex_i |= 1u << (rt * 4 + q);
      }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int64_t j = jb + ct * 16;
      if (j < n_total && (row_flags[j] & DAL_ROW_EXCLUDED)) ex_j |= 1u << ct;
    }
  }
  unsigned long long hits = 0;  // bit (rt * 4 + ct) * 4 + q
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t i = ib + rt * 16 + q, j = jb + ct * 16;
        const bool ok = acc[rt][ct][q] >= thr_scaled && i < j && j < n_total &&
                        !((ex_i >> (rt * 4 + q)) & 1u) && !((ex_j >> ct) & 1u);
        hits |= static_cast<unsigned long long>(ok) << ((rt * 4 + ct) * 4 + q);
      }
  const unsigned mine = static_cast<unsigned>(__builtin_popcountll(hits));
  // inclusive prefix over the wave's lanes
  unsigned incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned up = static_cast<unsigned>(__shfl_up(static_cast<int>(incl), d, 64));
    if (lane >= d) incl += up;
  }
  const unsigned total = static_cast<unsigned>(__shfl(static_cast<int>(incl), 63, 64));
  if (total == 0) return;
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(count, static_cast<unsigned long long>(total));
  const unsigned blo = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(base)));
  const unsigned bhi = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(base >> 32)));
  base = (static_cast<unsigned long long>(bhi) << 32) | blo;
  if (lane == 0 && base + total > static_cast<unsigned long long>(cap)) atomicOr(dev_status, DAL_FLAG_CAND_OVERFLOW);
  unsigned long long pos = base + (incl - mine);
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if ((hits >> ((rt * 4 + ct) * 4 + q)) & 1ull) {
          if (pos < static_cast<unsigned long long>(cap)) {
            const unsigned long long i = static_cast<unsigned long long>(ib + rt * 16 + q);
            const unsigned long long j = static_cast<unsigned long long>(jb + ct * 16);
            keys[pos] = (i << 32) | j;
            approx[pos] = acc[rt][ct][q] * 0x1p-24f;
          }
          ++pos;
        }
      }
}

__global__ __launch_bounds__(256) void pairs_resolve_kernel(const float* __restrict__ x, int64_t n, int64_t d,
                                                            int64_t ldx,
                                                            const double* __restrict__ norm64,
                                                            const unsigned long long* __restrict__ keys,
                                                            int64_t n_cand, double* __restrict__ values) {
  const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= n_cand) return;
  const unsigned long long key = keys[c];
  const int64_t i = static_cast<int64_t>(key >> 32), j = static_cast<int64_t>(key & 0xFFFFFFFFull);
  if (i >= n || j >= n) {  // not a key of this pool
    values[c] = __builtin_nan("");
    return;
  }
  const double ni = norm64[i], nj = norm64[j];
  const float* xi = x + i * ldx;
  const float* xj = x + j * ldx;
  double s = 0.0;
  for (int64_t f = 0; f < d; ++f) {
    const double ui = static_cast<double>(xi[f]) / ni;
    const double uj = static_cast<double>(xj[f]) / nj;
    s = s + ui * uj;  // -ffp-contract=off: multiply, then add (the canonical order)
  }
  values[c] = s;
}

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" double dal_cosine_pairs_error_bound(int64_t d_pad) {
  // |filter value - canonical cosine| for one pair (i, j) of rows with nonzero
  // norm, d_pad features (the padding features hold zeros).
  //
  // Operand.  u is the canonical fp64 unit row x / ||x||, v = fp32(u) its fp32
  // rounding (|v - u| <= 2^-24 |u|), H = fp16_rn(2^12 v).  For 2^12 |v| in the
  // fp16 normal range |H - 2^12 v| <= 2^-11 |2^12 v|; below it (|2^12 v| <
  // 2^-14) fp16 is spaced 2^-24 and |H - 2^12 v| <= 2^-25.  So h = 2^-12 H = u
  // + e with |e| <= delta |u| + eta, delta = 2^-11 (1 + 2^-24) + 2^-24 <
  // 2^-11 + 2^-23 and eta = 2^-37 (the subnormal range).
  //
  // Exact arithmetic.  sum_f h_if h_jf - sum_f u_if u_jf = sum (u_i e_j + e_i
  // u_j + e_i e_j).  With ||u|| <= 1 + 2^-40 =: r (the canonical rows are unit
  // up to fp64 rounding) and sum_f |u_f| <= r sqrt(d_pad) =: s1
  // (Cauchy-Schwarz):
  //   |sum u_i e_j| <= delta r^2 + eta s1              (and the same for e_i u_j)
  //   |sum e_i e_j| <= delta^2 r^2 + 2 delta eta s1 + eta^2 d_pad
  //
  // Accumulation.  Every product H_i H_j is exact in fp32 (two 11-bit
  // significands); the MFMAs add the d_pad products in fp32 in an order this
  // bound does not rely on: any order is within gamma_(d_pad) sum |h_i h_j| of
  // the exact sum, gamma_n = n u / (1 - n u), u = 2^-23 (the conservative unit
  // roundoff dal_density_error_bound_sym_d charges the MFMA's internal adds
  // with), and sum |h_i h_j| <= ||h_i|| ||h_j|| <= (r (1 + delta) + eta
  // sqrt(d_pad))^2.  The scaling by 2^-24 is exact.
  //
  // The canonical value itself is an fp64 sequential sum: within d_pad 2^-52 of
  // the real-number sum the terms above are measured against; charged 1e-12.
  //
  // d_pad 32: 9.81e-4, d_pad 1024: 1.10e-3 -- about 2^-10, the two fp16
  // roundings 2 x 2^-11.
  const double dp = static_cast<double>(d_pad > 0 ? d_pad : 0);
  const double delta = 0x1p-11 + 0x1p-23, eta = 0x1p-37, r = 1.0 + 0x1p-40;
  const double s1 = r * sqrt(dp);
  const double cross = 2.0 * (delta * r * r + eta * s1);
  const double quad = delta * delta * r * r + 2.0 * delta * eta * s1 + eta * eta * dp;
  const double u = 0x1p-23;
  const double gamma = dp * u / (1.0 - dp * u);
  const double hn = r * (1.0 + delta) + eta * sqrt(dp);
  return cross + quad + gamma * hn * hn + 1e-12;
}

extern "C" int dal_cosine_pairs(const uint16_t* rows, int64_t row_block0, int64_t n_row_blocks, const uint16_t* cols,
                                int64_t col_block0, int64_t j_lo, int64_t j_hi, int64_t n_total, int64_t d_pad,
                                const uint8_t* row_flags, double threshold, int64_t cap, uint64_t* keys, float* approx,
                                unsigned long long* count, int32_t* dev_status, dal_stream_t stream) {
  if (!rows || !cols || !keys || !approx || !count || !dev_status) return DAL_ERR_ARG;
  if (row_block0 < 0 || n_row_blocks <= 0 || col_block0 < 0 || n_total <= 0) return DAL_ERR_SHAPE;
  if (n_total > (int64_t{1} << 31) - 512) return DAL_ERR_SHAPE;  // row indices are packed in 32 bits
  const int64_t nb = dal_pad_rows(n_total) / kPairBlock;
  if (j_lo < col_block0 || j_hi < j_lo || j_hi > nb) return DAL_ERR_SHAPE;
  if (d_pad <= 0 || d_pad != dal_pad_features(d_pad) || d_pad > 1024) return DAL_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(cols)) & 15) return DAL_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(keys) & 7) || (reinterpret_cast<uintptr_t>(approx) & 3) ||
      (reinterpret_cast<uintptr_t>(count) & 7) || (reinterpret_cast<uintptr_t>(dev_status) & 3))
    return DAL_ERR_SHAPE;
  if (!(threshold == threshold) || threshold - threshold != 0.0 || cap < 0) return DAL_ERR_SHAPE;
  // row blocks past the pool hold no rows
  if (row_block0 >= nb) return DAL_OK;
  if (row_block0 + n_row_blocks > nb) n_row_blocks = nb - row_block0;
  const PairSchedule sched(row_block0, n_row_blocks, j_lo, j_hi);
  if (sched.total == 0) return DAL_OK;
  // one block per tile, as a 2-D grid of rows of kPairGridX blocks (a grid
  // dimension holds fewer than 2^32 threads; the last row's surplus blocks return)
  constexpr int64_t kPairGridX = 1 << 16;
  if (ceil_div(sched.tiles(), kPairGridX) > 65535) return DAL_ERR_CAPACITY;  // split the ranges
  // (tau - bound) 2^24 in fp32, rounded towards -inf (the power of two is exact)
  const double t = threshold - dal_cosine_pairs_error_bound(d_pad);
  float tf = static_cast<float>(t);
  if (static_cast<double>(tf) > t) tf = nextafterf(tf, -INFINITY);
  const float thr_scaled = tf * 0x1p24f;
  const int ks = split_ks(d_pad);
  const dim3 grid(static_cast<unsigned>(sched.tiles() < kPairGridX ? sched.tiles() : kPairGridX),
                  static_cast<unsigned>(ceil_div(sched.tiles(), kPairGridX)));
  hipStream_t st = as_stream(stream);
  if (d_pad == 32)
    hipLaunchKernelGGL(pairs_filter_kernel<32>, grid, dim3(kPairThreads), 0, st, rows, row_block0, n_row_blocks, cols,
                       col_block0, j_lo, j_hi, n_total, static_cast<int>(d_pad), ks, row_flags, thr_scaled, cap,
                       reinterpret_cast<unsigned long long*>(keys), approx, count, dev_status);
  else
    hipLaunchKernelGGL(pairs_filter_kernel<64>, grid, dim3(kPairThreads), 0, st, rows, row_block0, n_row_blocks, cols,
                       col_block0, j_lo, j_hi, n_total, static_cast<int>(d_pad), ks, row_flags, thr_scaled, cap,
                       reinterpret_cast<unsigned long long*>(keys), approx, count, dev_status);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

extern "C" int dal_cosine_pairs_resolve(const float* x, int64_t n, int64_t d, int64_t ldx, const double* norm64,
                                        const uint64_t* keys, int64_t n_cand, double* values, dal_stream_t stream) {
  if (!x || !norm64 || !keys || !values) return DAL_ERR_ARG;
  if (n <= 0 || d <= 0 || ldx < d || n_cand < 0) return DAL_ERR_SHAPE;
  if (n_cand > (int64_t{1} << 32) - 512) return DAL_ERR_CAPACITY;  // one thread per candidate, one grid dimension
  if ((reinterpret_cast<uintptr_t>(keys) & 7) || (reinterpret_cast<uintptr_t>(values) & 7)) return DAL_ERR_SHAPE;
  if (n_cand == 0) return DAL_OK;
  hipLaunchKernelGGL(pairs_resolve_kernel, dim3(static_cast<unsigned>(ceil_div(n_cand, 256))), dim3(256), 0,
                     as_stream(stream), x, n, d, ldx, norm64, reinterpret_cast<const unsigned long long*>(keys), n_cand,
                     values);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}
