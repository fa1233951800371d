// K13: greedy k-center (farthest-first) batch selection over a bf16 pool.
//
// Canonical definition (oracle max_cosine_canonical's cosine): with
//   m_i(0) = max_{l in L} cos64(i, l),
// step t = 1..k picks p_t = argmin over the live candidates of m_i(t-1) (ties
// -> lower global index), reports s_t = m_{p_t}(t-1), and then
//   m_i(t) = max(m_i(t-1), cos64(i, p_t))   for every row.
//
// Device state across the k steps: fp32 m32[n] within B = dal_kcenter_error_
// bound(d) of m_i(t) at every step, the row flags (DAL_ROW_CANDIDATE, and
// DAL_ROW_PICKED once picked), the centers table of canonical fp64 unit rows
// (feature-major [d][m + k]: the labeled rows, then each pick), the per-block
// minima of m32 over the live candidates, and the outputs.
//
// A step is propose (the shard's best row, as a record) and commit (the pick
// among the records of all shards, then the update pass).  The single-device
// selection is the same entries with one record.  Launches per step:
//   kc_mu        1 block     block minima -> mu, the contender threshold
//   kc_scan      nb blocks   blocks whose minimum reaches the threshold list
//                            their contenders (m32 <= mu + 2B)
//   kc_canon     fixed grid  one wave per contender: its canonical m_i(t-1)
//                            over the first m + t - 1 columns of the table
//   kc_record    1 block     the minimum (key, index) -> the record
//   kc_commit    1 block     the pick over the records; out_idx / out_score;
//                            the picked flag; the table's next column
//   kc_update    nb blocks   THE pass over the pool: m32 = max(m32, cos32) and
//                            the block minima of the next step
// Only kc_update reads the pool (n d 2 bytes, each row once); the others touch
// at most m32 and the flags (kc_scan: 5 n bytes when every block holds a
// contender, a few blocks' worth otherwise), the contenders' own rows, and the
// table.
//
// The bound B.  An fp32 value within B of its canonical counterpart, maximised
// against another such value, is within B of the canonical maximum, so the
// bound does not grow over the steps: B is the larger of the bound of m32(0)
// (dal_max_cosine: dal_maxcos_error_bound(d) = (3d + 6) u, u = 2^-24) and the
// bound of one step's cos32.  The step computes, for the pick's canonical unit
// row p (fp64) rounded once to fp32, p32_f = p_f (1 + e_f), |e_f| <= u:
//   dot32 = fl(sum_f x_if p32_f)   bf16 x_if exact in fp32; per lane an 8-term
//           FMA chain, then log2(d / 8) pairwise adds: every term passes
//           through at most 8 + 5 <= d roundings, each relative u, so
//           |dot32 - sum_f x_if p32_f| <= g_d sum_f |x_if p32_f|,
//           g_d = d u / (1 - d u)  (the standard dot-product bound, any order)
//   cos32 = fl(dot32 * inv_i), inv_i = fl32(1 / ||x_i||) of the fp64 norm: two
//           more relative roundings (and 2^-52-sized terms of the fp64 norm).
// With sum_f |x_if p_f| <= ||x_i|| ||p|| = ||x_i|| (Cauchy-Schwarz; ||p|| = 1
// up to 2^-50) and |cos| <= 1:
//   |cos32 - cos64| <= (g_d (1 + u) + u) + 2 u (1 + ...) < (d + 3) u / (1 - (d + 3) u).
// The canonical fp64 sums themselves carry < d 2^-52 < 1e-13, inside the
// 1e-12 slack.  As for dal_max_cosine, the fp32 products must neither
// overflow nor fall into the subnormal range (rows with ||x|| in 2^+-60 are
// far inside).  (d + 3) u < (3d + 6) u for every d, so B is dal_max_cosine's
// bound; both terms are evaluated so that a change of either stays covered.
//
// The canonical recompute of a contender filters the table's columns by an
// fp32 dot of the two unit rows, both rounded to fp32: |fp32 dot - canonical|
// <= E(d) = (d + 4) u (d u for the chain in any order, 2 u for the two operand
// roundings, slack for second-order terms and the fp64 sum) -- for every d,
// where topk.hip's fixed 2^-16 equals the chain term alone at d = 256.  A
// column can hold the canonical maximum only if its fp32 dot is within 2 E of
// the largest fp32 dot seen so far; only those get the sequential fp64 sum.
//
// K14: the ranked mode (ranked batch-mode selection, Cardoso et al. 2017).
// dal_kcenter_ranked_attach switches a begun job to it.  With weights w_i in
// [0, 1] and one alpha in (0, 1] per job, every operation one IEEE fp64
// operation in this order (no FMA):
//   b = 1 - alpha,  c_i = b w_i,  g_i(t) = alpha (1 - m_i(t-1)) + c_i,
// step t picks p_t = argmax over the live candidates of g_i(t) (ties -> lower
// global index), reports s_t = g_{p_t}(t) and r_t = m_{p_t}(t-1), and updates m
// as above.  The device state is K13's plus c[n] (fp64, computed once by the
// attach) and, in place of the block minima of m32, the per-block fp64 maxima
// over the live candidates of
//   g~_i = alpha (1 - (double)m32_i) + c_i      (the same three operations).
// The same six launches per step, instantiated with RANKED = true: kc_update
// folds the block maxima (reading 8 n more bytes, c), kc_mu forms mu = max and
// the threshold mu - 2 B_g, kc_scan lists the live candidates with g~_i >= mu -
// 2 B_g, kc_canon turns a contender's canonical m_i into g_i and keeps (key =
// score_key(-g), value = g, similarity = m), kc_record writes the similarity
// into the record's reserved word, kc_commit also writes out_sim[t].  The
// plain instantiations (RANKED = false) are the code they were: the added
// kernel arguments follow the old ones and are never read.
//
// The bound B_g = alpha B + 2^-48 (dal_kcenter_ranked_error_bound).  (double)
// m32_i is exact and |m32_i - m_i| <= B, so in exact arithmetic the two
// expressions differ by alpha |m32_i - m_i| <= alpha B.  Each side rounds three
// times: 1 - m (a value in [-B, 2 + B]: at most 2^-52), the product with alpha
// <= 1 (at most 2^-52, and the earlier error is scaled by alpha <= 1), the sum
// with c_i in [0, 1] (a value below 4: at most 2^-51); 2^-50 per side, 2^-49
// for both, inside the 2^-48.  The canonical argmax i* is always on the list:
// for the row j that holds mu,
//   g~_i* >= g_i* - B_g >= g_j - B_g >= g~_j - 2 B_g = mu - 2 B_g,
// and kc_scan recomputes g~ with the very operations of the fold, so the row
// that holds mu passes its own test and the list is never empty while a live
// candidate exists.  At alpha = 1, b = 0 and c_i = 0: farthest-first on 1 - m.
// A live candidate whose weight is NaN, infinite or outside [0, 1] raises
// DAL_FLAG_NONFINITE in the status word (the picks then mean nothing; every
// comparison with a NaN is false, so no row is listed twice or out of range).
#include "common.hpp"

#include <cstring>

namespace dal {
namespace {

constexpr uint32_t kKcMagic = 0x4b43454eu;  // "KCEN"
constexpr int kKcRows = 1024;               // rows per block of kc_update / kc_scan (the block minima's granule)
constexpr int kKcCanonBlocks = 256;         // kc_canon: 256 blocks x 4 waves, contenders grid-strided over the waves
constexpr int kKcWaves = kKcCanonBlocks * 4;
constexpr int kKcJ = 4;  // table columns per lane and chunk in kc_canon

struct KcCtl {
  double thr;       // mu + 2B
  float mu;         // the minimum of m32 over the live candidates (+inf: none)
  uint32_t count;   // contenders listed by kc_scan
};

struct KcJob {
  uint32_t magic;
  int32_t d;
  const uint16_t* pool;
  int64_t n, ld, idx_base, m, k, nb;
  uint8_t* flags;
  float* m32;
  const float* inv;
  double* centers;
  int64_t* out_idx;
  double* out_score;
  int32_t* status;
  double bound;
  // workspace pieces
  KcCtl* ctl;
  float* pick32;     // [256] the pick's unit row in fp32 (NaN: no pick)
  float* bmin;       // [nb]
  uint64_t* wkey;    // [kKcWaves]
  int64_t* widx;     // [kKcWaves]
  double* wval;      // [kKcWaves]
  unsigned char* rec;  // the shard's own record (dal_kcenter_select)
  int32_t* list;     // [n]
  // ranked mode (dal_kcenter_ranked_attach; all zero in a plain job)
  int32_t ranked;
  double alpha;
  double bound_g;      // alpha bound + 2^-48
  const double* c;     // [n] (1 - alpha) w_i
  double* bmax;        // [nb] block maxima of g~ over the live candidates
  double* wsim;        // [kKcWaves] the canonical m of each wave's best contender
  double* out_sim;     // [k]
};
static_assert(sizeof(KcJob) <= DAL_KCENTER_JOB_BYTES, "DAL_KCENTER_JOB_BYTES holds a k-center job");

struct KcLayout {
  size_t ctl, pick32, bmin, wkey, widx, wval, rec, list, total;
};

inline KcLayout kc_layout(int64_t n, int64_t d) {
  KcLayout L;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 255) / 256 * 256;
    return at;
  };
  const int64_t nb = ceil_div(n, kKcRows);
  L.ctl = take(sizeof(KcCtl));
  L.pick32 = take(256 * 4);
  L.bmin = take(static_cast<size_t>(nb > 0 ? nb : 1) * 4);
  L.wkey = take(kKcWaves * 8);
  L.widx = take(kKcWaves * 8);
  L.wval = take(kKcWaves * 8);
  L.rec = take(DAL_KCENTER_RECORD_BYTES(d));
  L.list = take(static_cast<size_t>(n > 0 ? n : 1) * 4);
  L.total = o;
  return L;
}

__device__ __forceinline__ bool kc_live(uint8_t f) { return (f & DAL_ROW_CANDIDATE) && !(f & DAL_ROW_PICKED); }

// The ranked score alpha (1 - m) + c: three fp64 operations, each rounded once
// (the canonical g_i from the canonical m_i, g~_i from (double)m32_i).
__device__ __forceinline__ double kc_rank(double alpha, double m, double c) {
  return __dadd_rn(__dmul_rn(alpha, __dsub_rn(1.0, m)), c);
}

struct KcRankedLayout {
  size_t c, bmax, wsim, total;
};

inline KcRankedLayout kc_ranked_layout(int64_t n) {
  KcRankedLayout L;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 255) / 256 * 256;
    return at;
  };
  const int64_t nb = ceil_div(n, kKcRows);
  L.c = take(static_cast<size_t>(n > 0 ? n : 1) * 8);
  L.bmax = take(static_cast<size_t>(nb > 0 ? nb : 1) * 8);
  L.wsim = take(kKcWaves * 8);
  L.total = o;
  return L;
}

// c_i = (1 - alpha) w_i for every row, and the check of the live candidates'
// weights (finite, in [0, 1]).
__global__ __launch_bounds__(256) void kc_rank_prep_kernel(const double* __restrict__ weight,
                                                           const uint8_t* __restrict__ flags, int64_t n, double b,
                                                           double* __restrict__ c, int32_t* __restrict__ status) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r >= n) return;
  const double w = weight[r];
  c[r] = __dmul_rn(b, w);
  if (kc_live(flags[r]) && !(w >= 0.0 && w <= 1.0)) atomicOr(status, DAL_FLAG_NONFINITE);
}

// The sum of a row's LPR lane sums (LPR = 8, 16 or 32 aligned lanes), on every
// lane of the row, by DPP: the quad's two exchanges (lane ^ 1, lane ^ 2), then
// the mirrors of 8 and of 16 lanes -- after the quad steps every lane of a quad
// holds the quad's sum, so the mirrored partner (7 - i, 15 - i) supplies the
// other quad's / other half's sum -- and one cross-row exchange at LPR = 32.
// Both partners add the same two values, so the tree is fixed and every lane
// ends with the same bits.
template <int CTRL>
__device__ __forceinline__ float kc_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int LPR>
__device__ __forceinline__ float kc_row_sum(float acc) {
  acc = acc + kc_dpp<0xB1>(acc);   // quad_perm [1, 0, 3, 2]
  acc = acc + kc_dpp<0x4E>(acc);   // quad_perm [2, 3, 0, 1]
  acc = acc + kc_dpp<0x141>(acc);  // row_half_mirror
  if (LPR >= 16) acc = acc + kc_dpp<0x140>(acc);  // row_mirror
  if (LPR >= 32) acc = acc + __shfl_xor(acc, 16);
  return acc;
}

// The update pass and the fold of the block minima.  Block b owns rows
// [b kKcRows, (b + 1) kKcRows).  D / 8 lanes per row, one 16-B load each (the
// lanes of a row read its 2 D bytes contiguously; a lane's feature slice is the
// same for every row, so its 8 fp32 values of the pick stay in registers).
// Lane sums: FMA chain over the slice's 8 features in ascending order; row sum:
// kc_row_sum over the row's lanes: a fixed tree, the same bits whatever the
// grid.  The 1024 dots go through LDS so that m32,
// 1 / ||x|| and the flags are read and m32 written as whole vectors.
// UPDATE false (dal_kcenter_begin, dal_kcenter_ranked_attach): the fold alone.
// RANKED: the fold is the fp64 maximum of g~ over the live candidates (bmax)
// instead of the fp32 minimum of m32 (bmin).
template <int D, bool UPDATE, bool RANKED>
__global__ __launch_bounds__(256) void kc_update_kernel(const uint16_t* __restrict__ pool, int64_t n, int64_t ld,
                                                        const float* __restrict__ pick32,
                                                        const float* __restrict__ inv, const uint8_t* __restrict__ flags,
                                                        float* __restrict__ m32, float* __restrict__ bmin,
                                                        int32_t* __restrict__ status, const double* __restrict__ c,
                                                        double alpha, double* __restrict__ bmax) {
  constexpr int LPR = D / 8;       // lanes per row
  constexpr int RPP = 256 / LPR;   // rows per pass of the block
  constexpr int PASSES = kKcRows / RPP;
  constexpr int U = 8;             // loads in flight per thread
  __shared__ float s_dot[kKcRows];
  __shared__ float s_min[4];
  const int tid = threadIdx.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kKcRows;
  if (UPDATE) {
    const int sl = tid % LPR, rr = tid / LPR;
    float p[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) p[e] = pick32[sl * 8 + e];
    const uint16_t* base = pool + sl * 8;
    for (int ps = 0; ps < PASSES; ps += U) {
      uint4 q[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t row = row0 + static_cast<int64_t>(ps + u) * RPP + rr;
        q[u] = row < n ? *reinterpret_cast<const uint4*>(base + row * ld) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // little endian: feature 2e in the low half
          acc = __builtin_fmaf(__uint_as_float(w[e] << 16), p[2 * e], acc);
          acc = __builtin_fmaf(__uint_as_float(w[e] & 0xFFFF0000u), p[2 * e + 1], acc);
        }
        acc = kc_row_sum<LPR>(acc);
        if (sl == 0) s_dot[(ps + u) * RPP + rr] = acc;
      }
    }
    __syncthreads();
  }
  // epilogue: thread t owns rows row0 + 4 t .. + 3
  float lo = __builtin_inff();
  double hi = -__builtin_inf();
  const int64_t r4 = row0 + 4 * tid;
  if (r4 + 3 < n && (reinterpret_cast<uintptr_t>(flags) & 3) == 0) {
    float4 mv = *reinterpret_cast<const float4*>(m32 + r4);
    const uchar4 fl = *reinterpret_cast<const uchar4*>(flags + r4);
    if (UPDATE) {
      const float4 iv = *reinterpret_cast<const float4*>(inv + r4);
      const float4 dt = *reinterpret_cast<const float4*>(s_dot + 4 * tid);
      if (!(iv.x < __builtin_inff()) || !(iv.y < __builtin_inff()) || !(iv.z < __builtin_inff()) ||
          !(iv.w < __builtin_inff()))
        atomicOr(status, DAL_FLAG_ZERO_NORM);
      mv.x = __builtin_fmaxf(mv.x, dt.x * iv.x);
      mv.y = __builtin_fmaxf(mv.y, dt.y * iv.y);
      mv.z = __builtin_fmaxf(mv.z, dt.z * iv.z);
      mv.w = __builtin_fmaxf(mv.w, dt.w * iv.w);
      *reinterpret_cast<float4*>(m32 + r4) = mv;
    }
    if (RANKED) {
      const double4 cv = *reinterpret_cast<const double4*>(c + r4);  // c is 256-B aligned, r4 a multiple of 4
      if (kc_live(fl.x)) hi = __builtin_fmax(hi, kc_rank(alpha, static_cast<double>(mv.x), cv.x));
      if (kc_live(fl.y)) hi = __builtin_fmax(hi, kc_rank(alpha, static_cast<double>(mv.y), cv.y));
      if (kc_live(fl.z)) hi = __builtin_fmax(hi, kc_rank(alpha, static_cast<double>(mv.z), cv.z));
      if (kc_live(fl.w)) hi = __builtin_fmax(hi, kc_rank(alpha, static_cast<double>(mv.w), cv.w));
    } else {
      if (kc_live(fl.x)) lo = __builtin_fminf(lo, mv.x);
      if (kc_live(fl.y)) lo = __builtin_fminf(lo, mv.y);
      if (kc_live(fl.z)) lo = __builtin_fminf(lo, mv.z);
      if (kc_live(fl.w)) lo = __builtin_fminf(lo, mv.w);
    }
  } else {
    for (int e = 0; e < 4; ++e) {
      const int64_t r = r4 + e;
      if (r >= n) break;
      float v = m32[r];
      if (UPDATE) {
        const float iv = inv[r];
        if (!(iv < __builtin_inff())) atomicOr(status, DAL_FLAG_ZERO_NORM);
        v = __builtin_fmaxf(v, s_dot[4 * tid + e] * iv);
        m32[r] = v;
      }
      if (RANKED) {
        if (kc_live(flags[r])) hi = __builtin_fmax(hi, kc_rank(alpha, static_cast<double>(v), c[r]));
      } else {
        if (kc_live(flags[r])) lo = __builtin_fminf(lo, v);
      }
    }
  }
  if (RANKED) {  // (block-uniform)
    __shared__ double s_max[4];
    for (int o = 32; o > 0; o >>= 1) hi = __builtin_fmax(hi, __shfl_xor(hi, o));
    if ((tid & 63) == 0) s_max[tid >> 6] = hi;
    __syncthreads();
    if (tid == 0)
      bmax[blockIdx.x] = __builtin_fmax(__builtin_fmax(s_max[0], s_max[1]), __builtin_fmax(s_max[2], s_max[3]));
    return;
  }
  for (int o = 32; o > 0; o >>= 1) lo = __builtin_fminf(lo, __shfl_xor(lo, o));
  if ((tid & 63) == 0) s_min[tid >> 6] = lo;
  __syncthreads();
  if (tid == 0)
    bmin[blockIdx.x] = __builtin_fminf(__builtin_fminf(s_min[0], s_min[1]), __builtin_fminf(s_min[2], s_min[3]));
}

// mu = min of the block minima; the contender threshold mu + 2B; an empty list.
// RANKED: mu = max of the block maxima of g~ (fp64), the threshold mu - 2 B_g
// (bound = B_g; -inf with no live candidate: kc_scan then lists nothing, since
// no row passes the liveness test).
template <bool RANKED>
__global__ __launch_bounds__(256) void kc_mu_kernel(const float* __restrict__ bmin, int64_t nb, double bound,
                                                    KcCtl* __restrict__ ctl, const double* __restrict__ bmax) {
  __shared__ float s_min[4];
  const int tid = threadIdx.x;
  if (RANKED) {
    __shared__ double s_max[4];
    double hi = -__builtin_inf();
    for (int64_t b = tid; b < nb; b += 256) hi = __builtin_fmax(hi, bmax[b]);
    for (int o = 32; o > 0; o >>= 1) hi = __builtin_fmax(hi, __shfl_xor(hi, o));
    if ((tid & 63) == 0) s_max[tid >> 6] = hi;
    __syncthreads();
    if (tid == 0) {
      const double mu = __builtin_fmax(__builtin_fmax(s_max[0], s_max[1]), __builtin_fmax(s_max[2], s_max[3]));
      ctl->mu = static_cast<float>(mu);
      ctl->thr = mu - 2.0 * bound;
      ctl->count = 0u;
    }
    return;
  }
  float lo = __builtin_inff();
  for (int64_t b = tid; b < nb; b += 256) lo = __builtin_fminf(lo, bmin[b]);
  for (int o = 32; o > 0; o >>= 1) lo = __builtin_fminf(lo, __shfl_xor(lo, o));
  if ((tid & 63) == 0) s_min[tid >> 6] = lo;
  __syncthreads();
  if (tid == 0) {
    const float mu = __builtin_fminf(__builtin_fminf(s_min[0], s_min[1]), __builtin_fminf(s_min[2], s_min[3]));
    ctl->mu = mu;
    ctl->thr = static_cast<double>(mu) + 2.0 * bound;
    ctl->count = 0u;
  }
}

// The contenders: live candidates with m32 <= mu + 2B (compared in fp64; the
// canonical argmin i* is one: m32[i*] <= m_i* + B <= m_j + B <= m32[j] + 2B for
// the row j that holds mu).  A block whose minimum is above the threshold
// holds none and reads nothing else.  The list holds up to n rows: no
// overflow, whatever the pool.
// RANKED: live candidates with g~ >= mu - 2 B_g, g~ recomputed by the fold's
// own operations (see the top of the file).
template <bool RANKED>
__global__ __launch_bounds__(256) void kc_scan_kernel(const float* __restrict__ m32,
                                                      const uint8_t* __restrict__ flags, int64_t n,
                                                      const float* __restrict__ bmin, KcCtl* __restrict__ ctl,
                                                      int32_t* __restrict__ list, const double* __restrict__ bmax,
                                                      const double* __restrict__ c, double alpha) {
  const double thr = ctl->thr;
  if (RANKED) {
    if (!(bmax[blockIdx.x] >= thr)) return;
  } else {
    if (!(static_cast<double>(bmin[blockIdx.x]) <= thr)) return;
  }
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kKcRows;
  for (int e = 0; e < kKcRows / 256; ++e) {
    const int64_t r = row0 + e * 256 + threadIdx.x;
    if (RANKED) {
      if (r < n && kc_live(flags[r]) && kc_rank(alpha, static_cast<double>(m32[r]), c[r]) >= thr)
        list[atomicAdd(&ctl->count, 1u)] = static_cast<int32_t>(r);
    } else {
      if (r < n && kc_live(flags[r]) && static_cast<double>(m32[r]) <= thr) list[atomicAdd(&ctl->count, 1u)] = static_cast<int32_t>(r);
    }
  }
}

// The canonical m_i(t-1) of every contender, one wave per contender (grid-
// strided over the list): the contender's canonical unit row into LDS, lanes
// over the table's columns with kKcJ fp32 dots each, and the sequential fp64
// sum for the columns within 2 E of the running fp32 maximum (see the top of
// the file).  A wave keeps its minimum (key, global index).  RANKED: the key is
// that of -g_i, g_i = alpha (1 - m_i) + c_i from the canonical m_i (so the
// minimum key is the maximum g), the value g_i, and m_i is kept beside it
// (wsim; read only for a wave that has a key).
template <bool RANKED>
__global__ __launch_bounds__(256) void kc_canon_kernel(const uint16_t* __restrict__ pool, int d, int64_t ld,
                                                       int64_t idx_base, const double* __restrict__ centers,
                                                       int64_t stride, int64_t ncol, const KcCtl* __restrict__ ctl,
                                                       const int32_t* __restrict__ list, float near2,
                                                       uint64_t* __restrict__ wkey, int64_t* __restrict__ widx,
                                                       double* __restrict__ wval, const double* __restrict__ cw,
                                                       double alpha, double* __restrict__ wsim) {
  __shared__ double s_u[4][256];
  __shared__ float s_f[4][256];
  __shared__ __attribute__((aligned(16))) double s_p[4][256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int gw = blockIdx.x * 4 + wave;
  const uint32_t count = ctl->count;
  uint64_t bkey = DAL_KEY_NONE;
  int64_t bidx = -1;
  double bval = __builtin_nan("");
  double* su = s_u[wave];
  float* sf = s_f[wave];
  double* sp = s_p[wave];
  for (uint32_t c = gw; c < count; c += kKcWaves) {
    const int64_t row = list[c];
    const uint16_t* xr = pool + row * ld;
    const double nr = __builtin_sqrt(row_sq_norm_bf16(xr, d));  // sequential in f; the same on every lane
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int f = lane; f < d; f += 64) {
      const double v = static_cast<double>(bf16_bits_to_f32(xr[f])) / nr;
      su[f] = v;
      sf[f] = static_cast<float>(v);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    float run32 = -__builtin_inff();
    double best = -__builtin_inf();
    for (int64_t lb = 0; lb < ncol; lb += 64 * kKcJ) {
      int64_t l[kKcJ];
      bool ok[kKcJ];
      float a[kKcJ];
#pragma unroll
      for (int j = 0; j < kKcJ; ++j) {
        l[j] = lb + lane + 64 * j;
        ok[j] = l[j] < ncol;
        if (!ok[j]) l[j] = ncol - 1;
        a[j] = 0.f;
      }
      if (RANKED) {
        // The same FMA chains as below (ascending f per column), with the 16
        // loads of four features issued before their first use: left to itself
        // the scheduler serialises them in this instantiation (3 in flight
        // instead of 16; the propose of a step measured 2.5x the plain one).
        for (int f = 0; f < d; f += 4) {  // (d is a multiple of 64)
          double cv[4][kKcJ];
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < kKcJ; ++j) cv[u][j] = centers[static_cast<int64_t>(f + u) * stride + l[j]];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float uq = sf[f + u];
#pragma unroll
            for (int j = 0; j < kKcJ; ++j) a[j] = __builtin_fmaf(uq, static_cast<float>(cv[u][j]), a[j]);
          }
        }
      } else {
#pragma unroll 4
      for (int f = 0; f < d; ++f) {
        const float uq = sf[f];
#pragma unroll
        for (int j = 0; j < kKcJ; ++j)
          a[j] = __builtin_fmaf(uq, static_cast<float>(centers[static_cast<int64_t>(f) * stride + l[j]]), a[j]);
      }
      }
      float cm = -__builtin_inff();
#pragma unroll
      for (int j = 0; j < kKcJ; ++j)
        if (ok[j]) cm = __builtin_fmaxf(cm, a[j]);
      for (int o = 32; o > 0; o >>= 1) cm = __builtin_fmaxf(cm, __shfl_xor(cm, o));
      run32 = __builtin_fmaxf(run32, cm);
      const float thr = run32 - near2;
#pragma unroll
      for (int j = 0; j < kKcJ; ++j) {
        unsigned long long near = __ballot(ok[j] && a[j] >= thr);
        while (near) {  // (wave-uniform)
          const int src = __ffsll(static_cast<long long>(near)) - 1;
          near &= near - 1;
          const int64_t lr = lb + src + 64 * j;
          // lane f's rounded products, then the sequential sum over f (the
          // canonical roundings and order)
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          for (int f = lane; f < d; f += 64) sp[f] = su[f] * centers[static_cast<int64_t>(f) * stride + lr];
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          double acc = 0.0;
          for (int f = 0; f < d; ++f) acc = acc + sp[f];
          if (acc > best) best = acc;
        }
      }
    }
    const double val = RANKED ? kc_rank(alpha, best, cw[row]) : best;
    const uint64_t key = score_key(RANKED ? -val : val, DAL_ASCENDING);
    const int64_t gi = row + idx_base;
    if (key < bkey || (key == bkey && gi < bidx)) {
      bkey = key;
      bidx = gi;
      bval = val;
      if (RANKED && lane == 0) wsim[gw] = best;  // (stored at once: nothing more to carry over the column loop)
    }
  }
  if (lane == 0) {
    wkey[gw] = bkey;
    widx[gw] = bidx;
    wval[gw] = bval;
  }
}

// Record layout (DAL_KCENTER_RECORD_BYTES(d)): u64 key, i64 global index, f64
// value, u64 reserved (0; RANKED: the fp64 similarity m, NaN bits without a
// key), d bf16 values of the row.
template <bool RANKED>
__global__ __launch_bounds__(256) void kc_record_kernel(const uint64_t* __restrict__ wkey,
                                                        const int64_t* __restrict__ widx,
                                                        const double* __restrict__ wval,
                                                        const uint16_t* __restrict__ pool, int d, int64_t ld,
                                                        int64_t idx_base, unsigned char* __restrict__ rec,
                                                        const double* __restrict__ wsim) {
  __shared__ uint64_t s_key[256];
  __shared__ int64_t s_idx[256];
  __shared__ int s_at[256];
  const int tid = threadIdx.x;
  uint64_t key = DAL_KEY_NONE;
  int64_t idx = -1;
  int at = 0;
  for (int w = tid; w < kKcWaves; w += 256) {
    const uint64_t k2 = wkey[w];
    const int64_t i2 = widx[w];
    if (k2 != DAL_KEY_NONE && (k2 < key || (k2 == key && i2 < idx))) {
      key = k2;
      idx = i2;
      at = w;
    }
  }
  s_key[tid] = key;
  s_idx[tid] = idx;
  s_at[tid] = at;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      const uint64_t k2 = s_key[tid + o];
      const int64_t i2 = s_idx[tid + o];
      if (k2 != DAL_KEY_NONE && (k2 < s_key[tid] || (k2 == s_key[tid] && i2 < s_idx[tid]))) {
        s_key[tid] = k2;
        s_idx[tid] = i2;
        s_at[tid] = s_at[tid + o];
      }
    }
    __syncthreads();
  }
  key = s_key[0];
  idx = s_idx[0];
  uint64_t* head = reinterpret_cast<uint64_t*>(rec);
  uint16_t* rrow = reinterpret_cast<uint16_t*>(rec + 32);
  if (tid == 0) {
    head[0] = key;
    head[1] = static_cast<uint64_t>(key == DAL_KEY_NONE ? -1ll : idx);
    head[2] = key == DAL_KEY_NONE ? 0x7FF8000000000000ull
                                  : static_cast<uint64_t>(__double_as_longlong(wval[s_at[0]]));
    if (RANKED)
      head[3] = key == DAL_KEY_NONE ? 0x7FF8000000000000ull
                                    : static_cast<uint64_t>(__double_as_longlong(wsim[s_at[0]]));
    else
      head[3] = 0ull;
  }
  for (int f = tid; f < d; f += 256) rrow[f] = key == DAL_KEY_NONE ? uint16_t(0) : pool[(idx - idx_base) * ld + f];
}

// The pick: the minimum (key, index) over the records (the same bytes on
// every rank give the same pick); out_idx[t] / out_score[t]; the picked flag
// when the row is local; the table's column m + t = the pick's canonical unit
// row, and its fp32 rounding for the update pass.  No record with a key: index
// -1, a NaN score, and a NaN pick (the update pass then leaves m32 as it is).
// RANKED: out_sim[t] = the winning record's similarity word (NaN without one).
template <bool RANKED>
__global__ __launch_bounds__(256) void kc_commit_kernel(const unsigned char* __restrict__ records, int64_t n_records,
                                                        int d, int64_t t, int64_t idx_base, int64_t n,
                                                        uint8_t* __restrict__ flags, double* __restrict__ centers,
                                                        int64_t stride, int64_t m, float* __restrict__ pick32,
                                                        int64_t* __restrict__ out_idx, double* __restrict__ out_score,
                                                        double* __restrict__ out_sim) {
  __shared__ int64_t s_win;
  const int tid = threadIdx.x;
  const size_t rb = DAL_KCENTER_RECORD_BYTES(d);
  if (tid == 0) {
    uint64_t key = DAL_KEY_NONE;
    int64_t idx = -1, win = -1;
    for (int64_t r = 0; r < n_records; ++r) {
      const uint64_t* head = reinterpret_cast<const uint64_t*>(records + r * rb);
      const uint64_t k2 = head[0];
      const int64_t i2 = static_cast<int64_t>(head[1]);
      if (k2 != DAL_KEY_NONE && (k2 < key || (k2 == key && i2 < idx))) {
        key = k2;
        idx = i2;
        win = r;
      }
    }
    s_win = win;
    if (win < 0) {
      out_idx[t] = -1;
      out_score[t] = __builtin_nan("");
      if (RANKED) out_sim[t] = __builtin_nan("");
    } else {
      const uint64_t* head = reinterpret_cast<const uint64_t*>(records + win * rb);
      out_idx[t] = idx;
      out_score[t] = __longlong_as_double(static_cast<long long>(head[2]));
      if (RANKED) out_sim[t] = __longlong_as_double(static_cast<long long>(head[3]));
      const int64_t loc = idx - idx_base;
      if (loc >= 0 && loc < n) flags[loc] = flags[loc] | DAL_ROW_PICKED;
    }
  }
  __syncthreads();
  const int64_t win = s_win;
  if (tid >= d) return;
  if (win < 0) {
    centers[static_cast<int64_t>(tid) * stride + m + t] = 0.0;
    pick32[tid] = __builtin_nanf("");
    return;
  }
  const uint16_t* row = reinterpret_cast<const uint16_t*>(records + win * rb + 32);
  const double nr = __builtin_sqrt(row_sq_norm_bf16(row, d));
  const double v = static_cast<double>(bf16_bits_to_f32(row[tid])) / nr;
  centers[static_cast<int64_t>(tid) * stride + m + t] = v;
  pick32[tid] = static_cast<float>(v);
}

template <bool UPDATE, bool RANKED>
int kc_launch_update(const KcJob& J, hipStream_t st) {
  if (J.nb == 0) return DAL_OK;
  const dim3 grid(static_cast<unsigned>(J.nb)), block(256);
  if (J.d == 64)
    hipLaunchKernelGGL((kc_update_kernel<64, UPDATE, RANKED>), grid, block, 0, st, J.pool, J.n, J.ld, J.pick32, J.inv,
                       J.flags, J.m32, J.bmin, J.status, J.c, J.alpha, J.bmax);
  else if (J.d == 128)
    hipLaunchKernelGGL((kc_update_kernel<128, UPDATE, RANKED>), grid, block, 0, st, J.pool, J.n, J.ld, J.pick32, J.inv,
                       J.flags, J.m32, J.bmin, J.status, J.c, J.alpha, J.bmax);
  else
    hipLaunchKernelGGL((kc_update_kernel<256, UPDATE, RANKED>), grid, block, 0, st, J.pool, J.n, J.ld, J.pick32, J.inv,
                       J.flags, J.m32, J.bmin, J.status, J.c, J.alpha, J.bmax);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

// One step's propose launches (see the top of the file).
template <bool RANKED>
int kc_launch_propose(const KcJob& J, int64_t t, unsigned char* record, hipStream_t st) {
  hipLaunchKernelGGL(kc_mu_kernel<RANKED>, dim3(1), dim3(256), 0, st, J.bmin, J.nb, RANKED ? J.bound_g : J.bound, J.ctl,
                     J.bmax);
  DAL_RETURN_IF_LAUNCH_FAILED();
  if (J.nb > 0) {
    hipLaunchKernelGGL(kc_scan_kernel<RANKED>, dim3(static_cast<unsigned>(J.nb)), dim3(256), 0, st, J.m32, J.flags, J.n,
                       J.bmin, J.ctl, J.list, J.bmax, J.c, J.alpha);
    DAL_RETURN_IF_LAUNCH_FAILED();
  }
  const float near2 = static_cast<float>(2.0 * (static_cast<double>(J.d) + 4.0) / 16777216.0);
  hipLaunchKernelGGL(kc_canon_kernel<RANKED>, dim3(kKcCanonBlocks), dim3(256), 0, st, J.pool, J.d, J.ld, J.idx_base,
                     J.centers, J.m + J.k, J.m + t, J.ctl, J.list, near2, J.wkey, J.widx, J.wval, J.c, J.alpha, J.wsim);
  DAL_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(kc_record_kernel<RANKED>, dim3(1), dim3(256), 0, st, J.wkey, J.widx, J.wval, J.pool, J.d, J.ld,
                     J.idx_base, record, J.wsim);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

// One step's commit launches: the pick, then the update pass.
template <bool RANKED>
int kc_launch_commit(const KcJob& J, int64_t t, const unsigned char* records, int64_t n_records, hipStream_t st) {
  hipLaunchKernelGGL(kc_commit_kernel<RANKED>, dim3(1), dim3(256), 0, st, records, n_records, J.d, t, J.idx_base, J.n,
                     J.flags, J.centers, J.m + J.k, J.m, J.pick32, J.out_idx, J.out_score, J.out_sim);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return kc_launch_update<true, RANKED>(J, st);
}

// A job read from caller memory (any alignment) and a step inside [0, k).
int kc_job_load(const void* job, int64_t t, KcJob* J) {
  if (!job) return DAL_ERR_ARG;
  std::memcpy(J, job, sizeof(KcJob));
  if (J->magic != kKcMagic) return DAL_ERR_ARG;
  if (t < 0 || t >= J->k) return DAL_ERR_SHAPE;
  return DAL_OK;
}

double kc_step_bound(int64_t d) {
  const double u = 1.0 / 16777216.0;
  const double k = static_cast<double>(d) + 3.0;
  return k * u / (1.0 - k * u) * 1.01 + 1e-12;
}

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" double dal_kcenter_error_bound(int64_t d) {
  const double a = dal_maxcos_error_bound(d), b = kc_step_bound(d);
  return a > b ? a : b;
}

extern "C" size_t dal_kcenter_workspace_bytes(int64_t n, int64_t d, int64_t m, int64_t k) {
  if (n < 0 || n > 0x7FFFFFFF || (d != 64 && d != 128 && d != 256) || m < 1 || k < 1) return 0;
  return kc_layout(n, d).total;
}

extern "C" int dal_kcenter_begin(void* job, const uint16_t* pool, int64_t n, int64_t d, int64_t ld, int64_t idx_base,
                                 uint8_t* row_flags, float* m32, const float* inv_norm, double* centers, int64_t m,
                                 int64_t k, void* ws, size_t ws_bytes, int64_t* out_idx, double* out_score,
                                 int32_t* dev_status, dal_stream_t stream) {
  if (!job) return DAL_ERR_ARG;
  std::memset(job, 0, sizeof(KcJob));  // a refused begin leaves no job behind
  if (!centers || !ws || !out_idx || !out_score || !dev_status) return DAL_ERR_ARG;
  if (n > 0 && (!pool || !row_flags || !m32 || !inv_norm)) return DAL_ERR_ARG;
  if (d != 64 && d != 128 && d != 256) return DAL_ERR_SHAPE;
  if (n < 0 || n > 0x7FFFFFFF || ld < d || ld % 8 || m < 1 || k < 1 || idx_base < 0) return DAL_ERR_SHAPE;
  if (m + k > 0x7FFFFFFF) return DAL_ERR_CAPACITY;
  if ((reinterpret_cast<uintptr_t>(pool) | reinterpret_cast<uintptr_t>(m32) | reinterpret_cast<uintptr_t>(inv_norm)) & 15)
    return DAL_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(centers) & 7) || (reinterpret_cast<uintptr_t>(ws) & 255)) return DAL_ERR_SHAPE;
  const KcLayout L = kc_layout(n, d);
  if (ws_bytes < L.total) return DAL_ERR_SHAPE;
  KcJob J;
  std::memset(&J, 0, sizeof J);
  J.magic = kKcMagic;
  J.d = static_cast<int32_t>(d);
  J.pool = pool;
  J.n = n;
  J.ld = ld;
  J.idx_base = idx_base;
  J.m = m;
  J.k = k;
  J.nb = ceil_div(n, kKcRows);
  J.flags = row_flags;
  J.m32 = m32;
  J.inv = inv_norm;
  J.centers = centers;
  J.out_idx = out_idx;
  J.out_score = out_score;
  J.status = dev_status;
  J.bound = dal_kcenter_error_bound(d);
  unsigned char* w = static_cast<unsigned char*>(ws);
  J.ctl = reinterpret_cast<KcCtl*>(w + L.ctl);
  J.pick32 = reinterpret_cast<float*>(w + L.pick32);
  J.bmin = reinterpret_cast<float*>(w + L.bmin);
  J.wkey = reinterpret_cast<uint64_t*>(w + L.wkey);
  J.widx = reinterpret_cast<int64_t*>(w + L.widx);
  J.wval = reinterpret_cast<double*>(w + L.wval);
  J.rec = w + L.rec;
  J.list = reinterpret_cast<int32_t*>(w + L.list);
  std::memcpy(job, &J, sizeof J);
  return kc_launch_update<false, false>(J, as_stream(stream));
}

extern "C" int dal_kcenter_propose(const void* job, int64_t t, void* record, dal_stream_t stream) {
  KcJob J;
  const int rc = kc_job_load(job, t, &J);
  if (rc != DAL_OK) return rc;
  if (!record || (reinterpret_cast<uintptr_t>(record) & 15)) return DAL_ERR_ARG;
  unsigned char* rec = static_cast<unsigned char*>(record);
  return J.ranked ? kc_launch_propose<true>(J, t, rec, as_stream(stream))
                  : kc_launch_propose<false>(J, t, rec, as_stream(stream));
}

extern "C" int dal_kcenter_commit(const void* job, int64_t t, const void* records, int64_t n_records,
                                  dal_stream_t stream) {
  KcJob J;
  const int rc = kc_job_load(job, t, &J);
  if (rc != DAL_OK) return rc;
  if (!records || (reinterpret_cast<uintptr_t>(records) & 15)) return DAL_ERR_ARG;
  if (n_records < 1) return DAL_ERR_SHAPE;
  const unsigned char* recs = static_cast<const unsigned char*>(records);
  return J.ranked ? kc_launch_commit<true>(J, t, recs, n_records, as_stream(stream))
                  : kc_launch_commit<false>(J, t, recs, n_records, as_stream(stream));
}

extern "C" int dal_kcenter_select(void* job, const uint16_t* pool, int64_t n, int64_t d, int64_t ld, int64_t idx_base,
                                  uint8_t* row_flags, float* m32, const float* inv_norm, double* centers, int64_t m,
                                  int64_t k, void* ws, size_t ws_bytes, int64_t* out_idx, double* out_score,
                                  int32_t* dev_status, dal_stream_t stream) {
  int rc = dal_kcenter_begin(job, pool, n, d, ld, idx_base, row_flags, m32, inv_norm, centers, m, k, ws, ws_bytes,
                             out_idx, out_score, dev_status, stream);
  if (rc != DAL_OK) return rc;
  return dal_kcenter_run(job, stream);
}

extern "C" int dal_kcenter_run(const void* job, dal_stream_t stream) {
  KcJob J;
  int rc = kc_job_load(job, 0, &J);
  if (rc != DAL_OK) return rc;
  for (int64_t t = 0; t < J.k; ++t) {
    if ((rc = dal_kcenter_propose(job, t, J.rec, stream)) != DAL_OK) return rc;
    if ((rc = dal_kcenter_commit(job, t, J.rec, 1, stream)) != DAL_OK) return rc;
  }
  return DAL_OK;
}

extern "C" size_t dal_kcenter_ranked_workspace_bytes(int64_t n) {
  if (n < 0 || n > 0x7FFFFFFF) return 0;
  return kc_ranked_layout(n).total;
}

extern "C" double dal_kcenter_ranked_error_bound(int64_t d, double alpha) {
  return alpha * dal_kcenter_error_bound(d) + 1.0 / 281474976710656.0;  // 2^-48
}

extern "C" int dal_kcenter_ranked_attach(void* job, const double* weight, double alpha, void* ws, size_t ws_bytes,
                                         double* out_sim, dal_stream_t stream) {
  KcJob J;
  const int rc = kc_job_load(job, 0, &J);  // (k >= 1 in every filled job: step 0 exists)
  if (rc != DAL_OK) return rc;
  if (!ws || !out_sim || (J.n > 0 && !weight)) return DAL_ERR_ARG;
  if (!(alpha > 0.0 && alpha <= 1.0)) return DAL_ERR_ARG;  // NaN included
  if ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(out_sim)) & 7) return DAL_ERR_SHAPE;
  if (reinterpret_cast<uintptr_t>(ws) & 255) return DAL_ERR_SHAPE;
  const KcRankedLayout L = kc_ranked_layout(J.n);
  if (ws_bytes < L.total) return DAL_ERR_SHAPE;
  unsigned char* w = static_cast<unsigned char*>(ws);
  double* c = reinterpret_cast<double*>(w + L.c);
  J.ranked = 1;
  J.alpha = alpha;
  J.bound_g = dal_kcenter_ranked_error_bound(J.d, alpha);
  J.c = c;
  J.bmax = reinterpret_cast<double*>(w + L.bmax);
  J.wsim = reinterpret_cast<double*>(w + L.wsim);
  J.out_sim = out_sim;
  std::memcpy(job, &J, sizeof J);
  if (J.nb == 0) return DAL_OK;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(kc_rank_prep_kernel, dim3(static_cast<unsigned>(ceil_div(J.n, 256))), dim3(256), 0, st, weight,
                     J.flags, J.n, 1.0 - alpha, c, J.status);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return kc_launch_update<false, true>(J, st);
}
