// The body of the blocked multiclass kernels (forest_multi_blocked.hip), included
// into forest_multi_blocked_kernel<NW, CW, DW, POW> and, with the step hooks,
// forest_multi_blocked_step_kernel<NW, CW, POW>: one text, two kernels.  A
// __device__ function called from both compiled the kernels without hooks to
// other instructions than they had (every one of the 24), by value, by
// reference, with and without __restrict__; included, they are the code they
// were.  In scope: NW, CW, DW, POW, STEP and the kernel's parameters A, xb,
// prep, fu_max, n_tiles.
//
// STEP (with DW; A is a McStepArgs): the first thread of the grid zeroes
// hooks.status_reset; the row leader's flags come from step_row_flag; and with
// hooks.gmin wave 0, which holds a tile's 64 rows on its lanes in the epilogue,
// folds the tile's minimum keys into row group tile / group_blocks -- two DPP
// wave minima, then lane 0's plain stores (group_blocks == 1) or atomic maxima
// of the inverted keys.  No barrier is added, wave 0 is the only writer, and
// in the four-wave kernels the atomics are left pending in thread 0's registers
// (McbFold) and issued after the next tile's DMA wait, as forest.hip's
// issue_fold does: issued at once they sat in wave 0's next s_waitcnt vmcnt(0),
// ahead of the barrier the whole block waits at.  The eight-wave kernels issue
// them at once, which measured faster there (kMcbDeferFold holds both figures).
  constexpr int NT = NW * 64;
  if constexpr (STEP) {
    if (A.hooks.status_reset && blockIdx.x == 0 && threadIdx.x == 0) *A.hooks.status_reset = 0;
  }
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
    // (forest.hip's loop)
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
  const int n_ins = blocked_dma_count(fu);  // DMA instructions per tile (4 runs each)
  typedef __attribute__((address_space(3))) float lds_float;
  typedef __attribute__((address_space(3))) const unsigned char lds_u8;
  const ByteWalk W{static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_u8*)fs)),
                   static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_u8*)ls)),
                   static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_float*)(xs + lane))),
                   NW, n_inner, n_leaf, A.depth};
  [[maybe_unused]] McbFold fold;  // STEP: thread 0's pending atomics (the four-wave kernels, kMcbDeferFold)
  constexpr bool DEFER = STEP && kMcbDeferFold && NW == kMcbWaves;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // block-uniform
    const int64_t row = tile * kBlk + lane;
    const bool live = row < A.n;
    const bool lead = wave == 0 && live;  // the rows' epilogue: wave 0
    // the row leader's flags (and, DW, its density word) are loaded with the tile
    uint8_t fl_pre = DAL_ROW_CANDIDATE;
    long long dens_pre = 0;
    if (lead) {
      if constexpr (STEP) fl_pre = step_row_flag(A.hooks, A.flags, row);
      else if (A.flags) fl_pre = A.flags[row];
      if constexpr (DW) dens_pre = static_cast<const long long*>(A.density)[row];
    }
    const char* src = reinterpret_cast<const char*>(xb + tile * A.d * kBlk);
    // (wave 0 stages nothing unless kMcbStageWave0)
    for (int i = kMcbStageWave0 ? wave : wave - 1; i >= 0 && i < n_ins; i += kMcbStageWave0 ? NW : NW - 1)
      stage_blocked_runs(xs, src, used, fu, i, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (DEFER) {
      // the previous tile's atomics, after this tile's DMA wait: they complete
      // under its walks instead of holding wave 0, and with it the block, there
      if (tid == 0) mcb_issue_fold(A.hooks, fold);
    }
    unsigned w[CW];
#pragma unroll
    for (int j = 0; j < CW; ++j) w[j] = 0u;
    if (live) {
      // groups of ILP trees, then the wave's last trees as ONE group of their
      // count; each tree's leaf byte is a class id, voted into w
      auto vote = [&](unsigned c) { add_vote<CW>(w, c); };
      for (int t = wave; t < A.n_trees; t += kMcbIlp * NW) {  // (wave-uniform)
        const int rem = (A.n_trees - t + NW - 1) / NW;
        if (rem >= kMcbIlp) walk_group<kMcbIlp>(W, t, vote);
        else walk_tail<kMcbIlp - 1>(W, t, rem, vote);
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
      if constexpr (STEP) {
        RowKeys K;  // (DAL_KEY_NONE on the last tile's dead lanes)
        if (live) K = row_epilogue<CW, DW, POW>(A, w, row, fl_pre, dens_pre, lut_s);
        if (A.hooks.gmin) {  // kernel-uniform
          // (32-bit tile arithmetic: n <= INT32_MAX, checked by the entry)
          const uint32_t gb = static_cast<uint32_t>(A.hooks.group_blocks), t32 = static_cast<uint32_t>(tile);
          const uint32_t g = t32 / gb;
          // the optimistic key carries the row's offset in its group (the select's prefetch hint)
          const unsigned long long klo = wave_min_u64_dpp(K.lo);
          const unsigned long long khi =
              wave_min_u64_dpp(pack_hint(K.hi, static_cast<long long>(t32 - g * gb) * kBlk + lane));
          if (lane == 0) {
            unsigned long long* lo_g = reinterpret_cast<unsigned long long*>(A.hooks.gmin) + g;
            unsigned long long* hi_g = lo_g + A.hooks.n_groups;
            if (gb == 1) {
              *lo_g = ~klo;
              *hi_g = ~khi;
            } else if (DEFER) {
              fold = McbFold{klo, khi, g, true};
            } else {
              if (klo != DAL_KEY_NONE) atomicMax(lo_g, ~klo);
              if (khi != DAL_KEY_NONE) atomicMax(hi_g, ~khi);
            }
          }
        }
      } else {
        if (live) row_epilogue<CW, DW, POW>(A, w, row, fl_pre, dens_pre, lut_s);
      }
    }
  }
  if constexpr (DEFER) {
    if (tid == 0) mcb_issue_fold(A.hooks, fold);  // the last tile's
  }
