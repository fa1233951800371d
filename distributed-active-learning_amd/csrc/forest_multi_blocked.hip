// Multiclass forest votes over the pool's blocked feature-major copy: the
// C-class form of forest.hip's prepared blocked kernel (forest_blocked_kernel
// <NW, PREP = true>), for the warm steps of a multiclass loop.
//
// Reference: as forest_multi.hip -- the per-tree predict and vote sum of
// final_thesis/uncertainty_sampling.py:88-97 for a forest of C classes, and
// the e*d product of density_weighting.py:148-167 for the density-weighted
// form.  The outputs are dal_forest_score_multiclass's and
// dal_forest_score_multiclass_dw's, bit for bit.
//
// MI355X design.  From the binary blocked kernel, as it is: a persistent grid;
// the forest prepared once per (forest, d) by dal_forest_prepare copied into
// LDS once per block, with the score LUT (T + 1 doubles) behind it; per 64-row
// tile only the runs of the features the forest tests, staged by
// global_load_lds_dwordx4, four 256-B runs per instruction; the rows on the 64
// lanes of every wave and the trees dealt over the NW waves (4, or 8 when a
// block's LDS lets at most two blocks onto a CU); byte-addressed walks, a
// select and a shift-add per level.  From forest_multi.hip: the votes as
// packed 8-bit fields in CW words (CW = 1, 2, 4, 8 for C <= 4, 8, 16, 32; every
// word index a compile-time constant) and the row leader's epilogue, the same
// arithmetic in the same order.  New here is only the cross-wave sum: a row's
// NW partial word sets sit in different waves, so waves 1 .. NW - 1 store
// theirs to an LDS exchange region ((NW - 1) CW words per row, lane-major: no
// bank conflicts) and wave 0 adds them field by field -- plain 32-bit adds, a
// field's total <= T <= 255 -- and runs the epilogue with lane = row.
//
// Two block barriers per tile: after the tile's DMA wait, and after the
// partial words are stored.  None closes the tile: every walk of tile k is
// over before its exchange barrier, so the other waves may stage tile k + 1
// while wave 0 writes tile k's rows out, and the exchange region is written
// again only after tile k + 1's DMA barrier, which wave 0 reaches after it
// has read tile k's words.
//
// LDS: [tile, fu_max runs of 256 B | prepared payload: nodes, leaves, feature
// list | LUT, round2(T + 1) doubles | exchange, (NW - 1) CW 256-B rows].
//
// The helpers below are copies of forest.hip's and forest_multi.hip's (not
// shared: those files' kernels are the code they were); the applicability rule
// is built on forest.hip's exported probes, so the two cannot drift apart.
#include <type_traits>

#include "common.hpp"

namespace dal {
namespace {

constexpr int kBlk = 64;        // rows per tile of the blocked copy (forest.hip)
constexpr int kMcbIlp = 4;      // independent tree walks in flight per lane
constexpr int kMcbPerCu = 5;    // blocks per CU at most (forest.hip, DAL_FOREST_BLOCKED_PER_CU)
constexpr int kMcbWaves = 4;
constexpr int kMcbWavesWide = 8;
#ifndef DAL_MCB_STAGE_WAVE0
#define DAL_MCB_STAGE_WAVE0 0
#endif
// Wave 0 takes a share of a tile's DMA instructions (1), or the other waves
// issue them all while wave 0 is still in the previous tile's epilogue (0).
// With its share wave 0 issued it only after that epilogue, and the whole block
// waited for those loads: config 4 (C = 10, T = 10) 221.8 -> 200.1 us, its
// density-weighted form 232.9 -> 227.3 us, config 2 12.06 -> 11.36 us, config 3
// 41.9 -> 41.8 us (the row-major kernel beside it 426 / 429 us in the two runs;
// profiles/multiclass/blocked_stage_wave0_summary.json holds the run with 1).
constexpr bool kMcbStageWave0 = DAL_MCB_STAGE_WAVE0 != 0;

// dal_forest_prepare's buffer (forest.hip, blocked_prep_layout): a 16-B header
// then [nodes int2 | leaves u8 round4 | feature list u16 round2(fu_max)],
// zero-padded to 16 B.
struct BlockedPrepLayout {
  int64_t nodes, leaves, used, payload, total;
};
__host__ __device__ inline BlockedPrepLayout blocked_prep_layout(int64_t n_trees, int32_t depth, int64_t fu_max) {
  BlockedPrepLayout L;
  L.nodes = n_trees * ((int64_t{1} << depth) - 1) * 8;
  L.leaves = round_up(n_trees << depth, 4);
  L.used = round_up(fu_max, 2) * 2;
  L.payload = round_up(L.nodes + L.leaves + L.used, 16);
  L.total = 16 + L.payload;
  return L;
}

struct McArgs {
  int64_t n;
  int d;
  int n_trees;
  int depth;
  int n_classes;
  const double* lut;
  int kind;
  const uint8_t* flags;
  int order;
  uint8_t* counts;
  uint8_t* pred;
  double* scores;
  uint64_t* keys;
  int cstore;  // bytes per store of a row's counts: 4, 2 or 1 (by C and the buffer's alignment)
};

struct McDwArgs : McArgs {
  const void* density;  // int64 fixed point (DAL_DENSITY_FIXED) or fp64 bits (DAL_DENSITY_EXACT), one word per row
  int dkind;
  double derr;
  double beta;
  double* entropy;
  int32_t* row_index;
  uint64_t* keys_hi;  // nullable
};

// pow out of line, and no call at all in the beta == 1 kernels (forest_multi.hip)
__device__ __attribute__((noinline)) double mcb_density_pow_general(double d, double beta) { return pow(d, beta); }
template <bool POW>
__device__ __forceinline__ double mcb_density_pow(double d, double beta) {
  if constexpr (POW) return mcb_density_pow_general(d, beta);
  return d;
}

// |d^beta - d'^beta| bound for |d - d'| <= derr.
__device__ __attribute__((noinline)) double mcb_density_pow_err_general(double d, double derr, double beta) {
  const double p = pow(fabs(d), beta);
  const double hi = pow(fabs(d) + derr, beta);
  const double lo = pow(fmax(fabs(d) - derr, 0.0), beta);
  return fmax(fabs(hi - p), fabs(p - lo)) * (1.0 + 1e-12) + fabs(p) * 1e-14;
}
template <bool POW>
__device__ __forceinline__ double mcb_density_pow_err(double d, double derr, double beta) {
  if constexpr (POW) return mcb_density_pow_err_general(d, derr, beta);
  return derr;
}

// One vote for class c: 1 << 8 (c & 3) added to word c >> 2, unrolled over the
// CW words; a class >= 4 CW matches no word and is dropped (forest_multi.hip).
template <int CW>
__device__ __forceinline__ void add_vote(unsigned (&w)[CW], unsigned c) {
  const unsigned inc = 1u << (8u * (c & 3u));
  const unsigned word = c >> 2;
#pragma unroll
  for (int j = 0; j < CW; ++j) w[j] += word == static_cast<unsigned>(j) ? inc : 0u;
}

template <int CW>
__device__ __forceinline__ int vote_field(const unsigned (&w)[CW], int c) {  // c: a compile-time constant at every call
  return static_cast<int>((w[c >> 2] >> (8 * (c & 3))) & 255u);
}

// Byte-addressed walks of M trees (t, t + tpr, ...) at once for one row
// (forest.hip, walk_group): node h of tree t sits at LDS byte tb + 8 h, so its
// child sits at 2a + (8 - tb) or 2a + (16 - tb); the leaf byte at (a >> 3) +
// lbase + t * n_leaf - n_inner - tb / 8.  Here each tree's leaf byte is a
// class id, voted into w.
struct ByteWalk {
  unsigned fbase, lbase, xb;  // LDS byte addresses: nodes, leaves, this row's x
  int tpr, n_inner, n_leaf, depth;
};
template <int M, int CW>
__device__ __forceinline__ void walk_group(const ByteWalk& W, int t, unsigned (&w)[CW]) {
  typedef __attribute__((address_space(3))) const float lds_float;
  typedef __attribute__((address_space(3))) const uint8_t lds_u8;
  typedef __attribute__((address_space(3))) const unsigned long long lds_u64;
  unsigned a[M], kl[M], kr[M], lo[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int tj = t + j * W.tpr;
    const unsigned tb = W.fbase + static_cast<unsigned>(8 * tj * W.n_inner);
    a[j] = tb;
    kl[j] = 8u - tb;
    kr[j] = 16u - tb;
    lo[j] = W.lbase + static_cast<unsigned>(tj * W.n_leaf - W.n_inner) - (tb >> 3);
    // opaque to the optimiser and held in vector registers, so the step stays
    // select + shift-add
    asm volatile("" : "+v"(kl[j]), "+v"(kr[j]));
  }
  for (int lvl = 0; lvl < W.depth; ++lvl) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const unsigned long long nd = *(lds_u64*)static_cast<uintptr_t>(a[j]);  // {feature run offset, thr}
      const float xv = *(lds_float*)static_cast<uintptr_t>(W.xb + static_cast<unsigned>(nd));
      a[j] = 2u * a[j] + (xv <= __uint_as_float(static_cast<unsigned>(nd >> 32)) ? kl[j] : kr[j]);
    }
  }
  unsigned c[M];
#pragma unroll
  for (int j = 0; j < M; ++j) c[j] = *(lds_u8*)static_cast<uintptr_t>((a[j] >> 3) + lo[j]);
#pragma unroll
  for (int j = 0; j < M; ++j) add_vote<CW>(w, c[j]);
}
// the last rem (< ILP) trees of a wave as one group (rem wave-uniform)
template <int M, int CW>
__device__ __forceinline__ void walk_tail(const ByteWalk& W, int t, int rem, unsigned (&w)[CW]) {
  if constexpr (M > 0) {
    if (rem == M) walk_group<M, CW>(W, t, w);
    else walk_tail<M - 1, CW>(W, t, rem, w);
  }
}

// The row leader's epilogue (forest_multi.hip, score_tile_multi from the
// cross-lane sum on): w holds the row's C counts.
template <int CW, bool DW, bool POW, class Args>
__device__ __forceinline__ void row_epilogue(const Args& A, const unsigned (&w)[CW], int64_t row, uint8_t fl_pre,
                                             long long dens_pre, const double* lut_s) {
  const int C = A.n_classes;
  // largest and second-largest count, the lowest class holding the largest
  int m1 = -1, m2 = -1, arg = 0;
#pragma unroll
  for (int c = 0; c < 4 * CW; ++c) {
    if (c < C) {
      const int nc = vote_field<CW>(w, c);
      if (nc > m1) {
        m2 = m1;
        m1 = nc;
        arg = c;
      } else if (nc > m2) {
        m2 = nc;
      }
    }
  }
  double s;
  if (DW || A.kind == DAL_MC_ENTROPY) {
    s = 0.0;
#pragma unroll
    for (int c = 0; c < 4 * CW; ++c)
      if (c < C) s = __dadd_rn(s, lut_s[vote_field<CW>(w, c)]);  // class order, one rounding per add
  } else {
    s = lut_s[A.kind == DAL_MC_MARGIN ? m1 - m2 : m1];
  }
  if (A.counts) {
    // the packed words are the row's count bytes in memory order (little
    // endian): whole words or halves where C and the buffer's alignment allow
    uint8_t* cr = A.counts + row * C;
    if (A.cstore == 4) {
#pragma unroll
      for (int j = 0; j < CW; ++j)
        if (4 * j < C) reinterpret_cast<uint32_t*>(cr)[j] = w[j];
    } else if (A.cstore == 2) {
#pragma unroll
      for (int hw = 0; hw < 2 * CW; ++hw)
        if (2 * hw < C) reinterpret_cast<uint16_t*>(cr)[hw] = static_cast<uint16_t>(w[hw >> 1] >> (16 * (hw & 1)));
    } else {
#pragma unroll
      for (int c = 0; c < 4 * CW; ++c)
        if (c < C) cr[c] = static_cast<uint8_t>(vote_field<CW>(w, c));
    }
  }
  if (A.pred) A.pred[row] = static_cast<uint8_t>(arg);
  if constexpr (DW) {
    // s = e d^beta, descending, and for the GEMM density the interval
    // s -+ e err(d^beta) as two keys
    const double e = s;
    double d = A.dkind == DAL_DENSITY_FIXED ? from_fixed(dens_pre) : __builtin_bit_cast(double, dens_pre);
    if (fl_pre & DAL_ROW_EXCLUDED) d = __builtin_nan("");
    s = e * mcb_density_pow<POW>(d, A.beta);
    double err = 0.0;
    if (A.dkind == DAL_DENSITY_FIXED && e != 0.0 && d == d) {
      err = e * mcb_density_pow_err<POW>(d, A.derr, A.beta);
      // keep the interval ends distinct from s after rounding
      err = fmax(err, fabs(s) * 4.5e-16);
    }
    unsigned long long klo = DAL_KEY_NONE, khi = DAL_KEY_NONE;
    if (fl_pre & DAL_ROW_CANDIDATE) {
      klo = score_key(pessimistic(s, err, DAL_DESCENDING), DAL_DESCENDING);
      khi = score_key(optimistic(s, err, DAL_DESCENDING), DAL_DESCENDING);
    }
    A.entropy[row] = e;
    A.row_index[row] = static_cast<int32_t>(row);  // (n <= INT32_MAX, checked by the entry)
    A.scores[row] = s;
    A.keys[row] = klo;
    if (A.keys_hi) A.keys_hi[row] = khi;
  } else {
    A.scores[row] = s;
    A.keys[row] = (fl_pre & DAL_ROW_CANDIDATE) ? score_key(s, A.order) : DAL_KEY_NONE;
  }
}

template <int NW, int CW, bool DW, bool POW>
__global__ __launch_bounds__(NW * 64) void forest_multi_blocked_kernel(std::conditional_t<DW, McDwArgs, McArgs> A,
                                                                       const float* __restrict__ xb,
                                                                       const unsigned char* __restrict__ prep,
                                                                       int fu_max, int64_t n_tiles) {
  constexpr int NT = NW * 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n_inner = (1 << A.depth) - 1, n_leaf = 1 << A.depth;
  const BlockedPrepLayout L = blocked_prep_layout(A.n_trees, A.depth, fu_max);
  float* xs = reinterpret_cast<float*>(smem);
  unsigned char* fs = smem + static_cast<size_t>(fu_max) * kBlk * 4;  // the prepared payload
  const uint8_t* ls = fs + L.nodes;
  const uint16_t* used = reinterpret_cast<const uint16_t*>(fs + L.nodes + L.leaves);
  double* lut_s = reinterpret_cast<double*>(fs + L.payload);                      // (16-B aligned)
  unsigned* ex = reinterpret_cast<unsigned*>(lut_s + round_up(A.n_trees + 1, 2));  // (16-B aligned)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i <= A.n_trees; i += NT) lut_s[i] = A.lut[i];
  {
    // the prepared payload -> LDS, 16 B per thread, kPrepBatch loads in flight
    constexpr int kPrepBatch = 4;
    const int n16 = static_cast<int>(L.payload >> 4);
    const uint4* src = reinterpret_cast<const uint4*>(prep + 16);
    uint4* dst = reinterpret_cast<uint4*>(fs);
    for (int e0 = tid; e0 < n16; e0 += kPrepBatch * NT) {
      uint4 q[kPrepBatch];
#pragma unroll
      for (int j = 0; j < kPrepBatch; ++j) q[j] = e0 + j * NT < n16 ? src[e0 + j * NT] : uint4{};
#pragma unroll
      for (int j = 0; j < kPrepBatch; ++j)
        if (e0 + j * NT < n16) dst[e0 + j * NT] = q[j];
    }
  }
  int fu = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(prep));
  fu = fu < fu_max ? fu : fu_max;  // (the buffer's own bound: the tile holds fu_max runs)
  __syncthreads();
  const int n_ins = (fu + 3) >> 2;  // DMA instructions per tile (4 runs each)
  typedef __attribute__((address_space(3))) float lds_float;
  typedef __attribute__((address_space(3))) const unsigned char lds_u8;
  const ByteWalk W{static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_u8*)fs)),
                   static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_u8*)ls)),
                   static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_float*)(xs + lane))),
                   NW, n_inner, n_leaf, A.depth};
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // block-uniform
    const int64_t row = tile * kBlk + lane;
    const bool live = row < A.n;
    const bool lead = wave == 0 && live;  // the rows' epilogue: wave 0
    // the row leader's flags (and, DW, its density word) are loaded with the tile
    uint8_t fl_pre = DAL_ROW_CANDIDATE;
    long long dens_pre = 0;
    if (lead) {
      if (A.flags) fl_pre = A.flags[row];
      if constexpr (DW) dens_pre = static_cast<const long long*>(A.density)[row];
    }
    const char* src = reinterpret_cast<const char*>(xb + tile * A.d * kBlk);
    // (wave 0 stages nothing unless kMcbStageWave0)
    for (int i = kMcbStageWave0 ? wave : wave - 1; i >= 0 && i < n_ins; i += kMcbStageWave0 ? NW : NW - 1) {
      const int sl = 4 * i + (lane >> 4);
      const unsigned dst = __builtin_amdgcn_readfirstlane(
          static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_float*)(xs + 4 * i * kBlk))));
      if (sl < fu) {
        const unsigned voff = static_cast<unsigned>(used[sl]) * (kBlk * 4u) + static_cast<unsigned>(lane & 15) * 16u;
        unsigned keep;
        asm volatile(
            "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(voff), "s"(dst), "s"(src)
            : "memory");
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned w[CW];
#pragma unroll
    for (int j = 0; j < CW; ++j) w[j] = 0u;
    if (live) {
      // groups of ILP trees, then the wave's last trees as ONE group of their count
      for (int t = wave; t < A.n_trees; t += kMcbIlp * NW) {  // (wave-uniform)
        const int rem = (A.n_trees - t + NW - 1) / NW;
        if (rem >= kMcbIlp) walk_group<kMcbIlp, CW>(W, t, w);
        else walk_tail<kMcbIlp - 1, CW>(W, t, rem, w);
      }
    }
    // a row's NW partial word sets, one per wave, added field by field
    // through LDS (a field's total <= T <= 255: no carry)
    if (wave != 0) {
#pragma unroll
      for (int j = 0; j < CW; ++j) ex[((wave - 1) * CW + j) * kBlk + lane] = w[j];
    }
    __syncthreads();  // ... and every walk of this tile is over: the next tile may be staged
    if (wave == 0) {
#pragma unroll
      for (int q = 0; q < NW - 1; ++q) {
#pragma unroll
        for (int j = 0; j < CW; ++j) w[j] += ex[(q * CW + j) * kBlk + lane];
      }
      if (live) row_epilogue<CW, DW, POW>(A, w, row, fl_pre, dens_pre, lut_s);
    }
  }
}

constexpr int mcb_words(int32_t n_classes) { return n_classes <= 4 ? 1 : n_classes <= 8 ? 2 : n_classes <= 16 ? 4 : 8; }

// The applicability rule and the launch shape.  The prepared forest is
// dal_forest_prepare's, so the rule starts from forest.hip's: a buffer exists
// (dal_forest_blocked_rows), fu_max = min(nodes, d) is its bound on the
// distinct features, and its size must be the one this file's copy of the
// layout gives.  The block's LDS is the tile, the payload, the LUT and the
// exchange region, within the 96 KiB the binary rule allows itself; 8 waves
// when four-wave blocks fit at most two per CU (the binary rule's threshold).
struct McbPlan {
  int fu_max = 0;  // 0: the blocked kernel does not apply
  int nw = 0;
  size_t smem = 0;
};
McbPlan mcb_plan(int64_t d, int32_t n_trees, int32_t depth, int32_t n_classes) {
  McbPlan P;
  if (n_classes < 2 || n_classes > DAL_MC_MAX_CLASSES || n_trees < 1 || n_trees > DAL_MC_MAX_TREES) return P;
  if (!dal_forest_blocked_rows(d, n_trees, depth)) return P;
  const int64_t nodes = static_cast<int64_t>(n_trees) * ((int64_t{1} << depth) - 1);
  const int64_t fu = nodes < d ? nodes : d;
  const BlockedPrepLayout L = blocked_prep_layout(n_trees, depth, fu);
  if (static_cast<size_t>(L.total) != dal_forest_prep_bytes(d, n_trees, depth)) return P;
  const size_t base = static_cast<size_t>(fu) * kBlk * 4 + static_cast<size_t>(L.payload) +
                      static_cast<size_t>(round_up(n_trees + 1, 2)) * 8;
  const size_t row_bytes = static_cast<size_t>(mcb_words(n_classes)) * kBlk * 4;  // one wave's partial words
  const bool wide = base + (kMcbWaves - 1) * row_bytes > (160u << 10) / 3;
  const int nw = wide ? kMcbWavesWide : kMcbWaves;
  const size_t smem = base + (nw - 1) * row_bytes;
  if (smem > 96 * 1024) return P;
  P.fu_max = static_cast<int>(fu);
  P.nw = nw;
  P.smem = smem;
  return P;
}

template <int CW, bool DW, bool POW, class Args>
int mcb_launch(const Args& A, const float* xb, const void* fprep, const McbPlan& P, hipStream_t st) {
  const int64_t tiles = ceil_div(A.n, kBlk);
  const bool wide = P.nw == kMcbWavesWide;
  const void* fn = wide ? reinterpret_cast<const void*>(forest_multi_blocked_kernel<kMcbWavesWide, CW, DW, POW>)
                        : reinterpret_cast<const void*>(forest_multi_blocked_kernel<kMcbWaves, CW, DW, POW>);
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1 ||
      hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(P.smem)) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, P.nw * 64, P.smem) != hipSuccess)
    return DAL_ERR_HIP;
  // a persistent grid of the blocks resident at once, kMcbPerCu per CU at
  // most: every block stages the forest once (forest.hip)
  if (per_cu > kMcbPerCu) per_cu = kMcbPerCu;
  if (per_cu < 1) per_cu = 1;
  const int64_t grid = tiles < static_cast<int64_t>(cus) * per_cu ? tiles : static_cast<int64_t>(cus) * per_cu;
  const unsigned char* pb = static_cast<const unsigned char*>(fprep);
  if (wide)
    hipLaunchKernelGGL((forest_multi_blocked_kernel<kMcbWavesWide, CW, DW, POW>), dim3(static_cast<unsigned>(grid)),
                       dim3(kMcbWavesWide * 64), P.smem, st, A, xb, pb, P.fu_max, tiles);
  else
    hipLaunchKernelGGL((forest_multi_blocked_kernel<kMcbWaves, CW, DW, POW>), dim3(static_cast<unsigned>(grid)),
                       dim3(kMcbWaves * 64), P.smem, st, A, xb, pb, P.fu_max, tiles);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

// The row-major entries' validation up to n == 0, then the blocked operands':
// DAL_OK means launch.
int mcb_validate(const float* x, const float* xb, const void* fprep, int64_t n, int64_t d, int64_t ldx, int32_t n_trees,
                 int32_t depth, int32_t n_classes) {
  if (n < 0 || d < 1 || ldx < d || d > (int64_t{1} << 30)) return DAL_ERR_SHAPE;
  if (depth < 1 || depth > DAL_MAX_TREE_DEPTH) return DAL_ERR_UNSUPPORTED;
  if (n_classes < 2 || n_classes > DAL_MC_MAX_CLASSES) return DAL_ERR_UNSUPPORTED;
  if (n_trees < 1 || n_trees > DAL_MC_MAX_TREES) return DAL_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(xb) % 16 != 0) return DAL_ERR_ARG;
  if (mcb_plan(d, n_trees, depth, n_classes).fu_max && (!fprep || reinterpret_cast<uintptr_t>(fprep) % 16 != 0))
    return DAL_ERR_ARG;
  return DAL_OK;
}

int mcb_cstore(const uint8_t* counts, int32_t n_classes) {
  const uintptr_t ca = reinterpret_cast<uintptr_t>(counts);
  return (n_classes % 4 == 0 && ca % 4 == 0) ? 4 : (n_classes % 2 == 0 && ca % 2 == 0) ? 2 : 1;
}

}  // namespace
}  // namespace dal

using namespace dal;

extern "C" int dal_forest_multiclass_blocked_rows(int64_t d, int32_t n_trees, int32_t depth, int32_t n_classes) {
  return mcb_plan(d, n_trees, depth, n_classes).fu_max ? kBlk : 0;
}

extern "C" int dal_forest_score_multiclass_blocked(const float* x, const float* xb, const void* fprep, int64_t n,
                                                   int64_t d, int64_t ldx, const int32_t* inner, const uint8_t* leaf,
                                                   int32_t n_trees, int32_t depth, int32_t n_classes,
                                                   const double* lut, int score_kind, const uint8_t* row_flags,
                                                   int order, uint8_t* counts, uint8_t* pred, double* scores,
                                                   uint64_t* keys, dal_stream_t stream) {
  if (!xb)
    return dal_forest_score_multiclass(x, n, d, ldx, inner, leaf, n_trees, depth, n_classes, lut, score_kind,
                                       row_flags, order, counts, pred, scores, keys, stream);
  if (!x || !inner || !leaf || !lut || !scores || !keys) return DAL_ERR_ARG;
  if (order != DAL_ASCENDING && order != DAL_DESCENDING) return DAL_ERR_ARG;
  if (score_kind != DAL_MC_LEAST_CONFIDENCE && score_kind != DAL_MC_MARGIN && score_kind != DAL_MC_ENTROPY)
    return DAL_ERR_ARG;
  if (const int rc = mcb_validate(x, xb, fprep, n, d, ldx, n_trees, depth, n_classes)) return rc;
  if (n == 0) return DAL_OK;
  const McbPlan P = mcb_plan(d, n_trees, depth, n_classes);
  if (!P.fu_max)
    return dal_forest_score_multiclass(x, n, d, ldx, inner, leaf, n_trees, depth, n_classes, lut, score_kind,
                                       row_flags, order, counts, pred, scores, keys, stream);
  const McArgs A{n,     static_cast<int>(d), n_trees, depth, n_classes, lut,  score_kind, row_flags,
                 order, counts,              pred,    scores, keys,     mcb_cstore(counts, n_classes)};
  const hipStream_t st = as_stream(stream);
  if (n_classes <= 4) return mcb_launch<1, false, false>(A, xb, fprep, P, st);
  if (n_classes <= 8) return mcb_launch<2, false, false>(A, xb, fprep, P, st);
  if (n_classes <= 16) return mcb_launch<4, false, false>(A, xb, fprep, P, st);
  return mcb_launch<8, false, false>(A, xb, fprep, P, st);
}

extern "C" int dal_forest_score_multiclass_dw_blocked(const float* x, const float* xb, const void* fprep, int64_t n,
                                                      int64_t d, int64_t ldx, const int32_t* inner,
                                                      const uint8_t* leaf, int32_t n_trees, int32_t depth,
                                                      int32_t n_classes, const double* lut, const void* density,
                                                      int density_kind, double density_err,
                                                      const uint8_t* row_flags, double beta, uint8_t* counts,
                                                      uint8_t* pred, double* entropy, int32_t* row_index,
                                                      double* scores, uint64_t* keys, uint64_t* keys_hi,
                                                      dal_stream_t stream) {
  if (!xb)
    return dal_forest_score_multiclass_dw(x, n, d, ldx, inner, leaf, n_trees, depth, n_classes, lut, density,
                                          density_kind, density_err, row_flags, beta, counts, pred, entropy,
                                          row_index, scores, keys, keys_hi, stream);
  if (!x || !inner || !leaf || !lut || !density || !entropy || !row_index || !scores || !keys) return DAL_ERR_ARG;
  if (density_kind != DAL_DENSITY_FIXED && density_kind != DAL_DENSITY_EXACT) return DAL_ERR_ARG;
  if (n > INT32_MAX) return DAL_ERR_SHAPE;  // row_index is int32 (dal_dw_select's vote type)
  if (const int rc = mcb_validate(x, xb, fprep, n, d, ldx, n_trees, depth, n_classes)) return rc;
  if (n == 0) return DAL_OK;
  const McbPlan P = mcb_plan(d, n_trees, depth, n_classes);
  if (!P.fu_max)
    return dal_forest_score_multiclass_dw(x, n, d, ldx, inner, leaf, n_trees, depth, n_classes, lut, density,
                                          density_kind, density_err, row_flags, beta, counts, pred, entropy,
                                          row_index, scores, keys, keys_hi, stream);
  const McDwArgs A{{n, static_cast<int>(d), n_trees, depth, n_classes, lut, DAL_MC_ENTROPY, row_flags, DAL_DESCENDING,
                    counts, pred, scores, keys, mcb_cstore(counts, n_classes)},
                   density, density_kind, density_err, beta, entropy, row_index, keys_hi};
  const hipStream_t st = as_stream(stream);
  if (beta == 1.0) {  // no pow, no call
    if (n_classes <= 4) return mcb_launch<1, true, false>(A, xb, fprep, P, st);
    if (n_classes <= 8) return mcb_launch<2, true, false>(A, xb, fprep, P, st);
    if (n_classes <= 16) return mcb_launch<4, true, false>(A, xb, fprep, P, st);
    return mcb_launch<8, true, false>(A, xb, fprep, P, st);
  }
  if (n_classes <= 4) return mcb_launch<1, true, true>(A, xb, fprep, P, st);
  if (n_classes <= 8) return mcb_launch<2, true, true>(A, xb, fprep, P, st);
  if (n_classes <= 16) return mcb_launch<4, true, true>(A, xb, fprep, P, st);
  return mcb_launch<8, true, true>(A, xb, fprep, P, st);
}
