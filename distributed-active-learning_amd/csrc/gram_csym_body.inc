// The body of the symmetric Gram kernels (gram_sym.hip): included by
// gram_csym_kernel<KS, W, HVS> and by the int8 and fp4 instances
// gram_i8sym_kernel and gram_fp4sym_kernel behind `using C = Cfg<...>;`, with the kernels' argument names.
  constexpr int HV = C::HALVES;
  __shared__ __attribute__((aligned(16))) float4 lds[2 * C::F4];
  __shared__ typename C::racc_t rowacc[HV * kSB];
  __shared__ int claim_lds[2];  // a claimed unit index, lane 0 -> the block (two words: see claim_begin)

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int half = wave / C::WPS, wave4 = wave % C::WPS;  // the block's super block of this wave, wave within it
  // 8-wave block: the two waves of a SIMD (w, w + 4) run the same program in
  // lockstep; a static priority for one half settles their VALU arbitration
  // once instead of by age at every segment (MI355X_MICROARCH.md, two waves per
  // SIMD): waves 4-7 at priority 1, 2M x 256 1266.9 -> 1262.3 ms (waves 0-3:
  // 1265.0; deferring waves 4-7's last column epilogue of each stage into the
  // next one, a stagger, 1274.5)
  if constexpr (C::WAVES == 8 && DAL_GRAM_PRIO8 != 0) {
    if (DAL_GRAM_PRIO8 > 0 ? wave >= 4 : wave < 4) __builtin_amdgcn_s_setprio(1);
  }
  const int li = lane & 15, lq = lane >> 4;
  const int G = gridDim.x, g = blockIdx.x;
  for (int e = tid; e < HV * kSB; e += C::NT) rowacc[e] = 0.0;

  // the pairs this block multiplies and their order: gram_schedule.hpp
  const GramSchedule<HV> sched(srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi, ns_active, chunk_j, n_chunks, contig, G,
                               g);

  // DMA source offsets.  Piece q of wave w covers stage rows
  // Wr + q * RPP + lane / SLOTS (Wr = w * PIECES * RPP, RPP = 64 / SLOTS rows
  // per piece), slot (lane % SLOTS) ^ swz(row).  Wr (a multiple of
  // PIECES * RPP), q * RPP and lane / SLOTS occupy disjoint bits, so at 8 and
  // 16 slots swz(row) = row & SWZ = swz(Wr + lane / SLOTS) ^ swz(q * RPP): the
  // offset is a per-lane value XOR a per-piece constant (bits 4.. of the byte
  // offset, below the row part) plus the piece's row offset.  At 4 slots a
  // piece is 16 rows and swz reads row bits 2-3 only: all in lane / SLOTS, the
  // per-piece constant is 0.
  constexpr int RPP = 64 / C::SLOTS;
  static_assert((RPP & (RPP - 1)) == 0 && (C::PIECES & (C::PIECES - 1)) == 0, "row parts must occupy disjoint bits");
  const unsigned rowbytes = static_cast<unsigned>(ldh * 2);
  const unsigned dst0 = __builtin_amdgcn_readfirstlane(
      static_cast<unsigned>(reinterpret_cast<uintptr_t>((AS3 float4*)(lds + wave * C::PIECES * 64))));
  // stage h of 256-column block J of feature slice `slice` into LDS buffer
  // buf.  Inline asm so the compiler does not track the DMA on vmcnt
  // (block_sync waits for it).
  auto issue = [&](int buf, int J, int h, int slice) {
    // (the cursor's values are uniform, but the compiler may hold them in
    // vector registers when the scalar ones run out: the asm needs scalars)
    J = __builtin_amdgcn_readfirstlane(J);
    slice = __builtin_amdgcn_readfirstlane(slice);
    const char* sbase = reinterpret_cast<const char*>(
        ucols + (static_cast<int64_t>(J - jcol0) * 256 + h * C::SC) * ldh + slice_off + C::sub_off(slice));
    const unsigned fl = fresh_lane();
    const unsigned lrow = fl / C::SLOTS + static_cast<unsigned>(wave * C::PIECES * RPP);
    const unsigned vlane = lrow * rowbytes + (((fl % C::SLOTS) ^ static_cast<unsigned>(C::swz(lrow))) << 4);
#pragma unroll
    for (int q = 0; q < C::PIECES; ++q) {
      const unsigned dst = dst0 + static_cast<unsigned>(buf * C::STAGE + q * 1024);
      const unsigned voff = (vlane ^ (static_cast<unsigned>(C::swz(q * RPP)) << 4)) +
                            static_cast<unsigned>(q * RPP) * rowbytes;
      lds_dma_x4(voff, dst, sbase);
    }
  };

  // resident A fragments: H of rows P*512 + wave4*RPW + rt*16 + (lane & 15)
  // (P = this wave's super block of the unit), features of k-step c and lane
  // group lq (the MFMA's N side; the staged column tile is its M side)
  f16x8 ah[C::RT][C::NKS];
  auto load_a = [&](int ru, int slice) {
    const int P = sched.rowP(ru, half);
    if (HV > 1 && !sched.live(P)) return;  // (this half idles for the unit)
    const uint16_t* pb = urows + static_cast<int64_t>(P - srow0) * kSB * ldh + slice_off + C::sub_off(slice);
    const unsigned fl = fresh_lane();
    const unsigned lrow = static_cast<unsigned>((wave4 * C::RPW + (fl & 15)) * ldh + (fl >> 4) * 8);
    const unsigned tstep = static_cast<unsigned>(16 * ldh);
#pragma unroll
    for (int rt = 0; rt < C::RT; ++rt)
#pragma unroll
      for (int c = 0; c < C::NKS; ++c)  // read once per unit: keep the column stages resident in L2
        ah[rt][c] = __builtin_nontemporal_load(reinterpret_cast<const f16x8*>(pb + lrow + rt * tstep + c * C::LG * 8));
  };
  // B-fragment LDS offsets (float4 units): slot (k + lq) ^ swz(li) of column
  // row li (a stage's tiles start at multiples of 16 rows: swz(row) = swz(li)),
  // k = c*LG a multiple of 4; the XOR splits into a lane part (low 2 bits) and
  // a k part (k ^ (swz(li) & ~3)), so two registers cover every k-step
  const int b_base = li * C::SLOTS + (lq ^ (C::swz(li) & 3));
  const int b_swz = C::swz(li) & ~3;
  auto b_off = [&](int c) { return b_base + ((c * C::LG) ^ b_swz); };

  typename C::acc4 mc[C::NCH][C::RT];
  constexpr bool kDefer = C::FOLD_PAIRS > 1;  // chains over several pairs (round 15, below)
  // the fp4 form's scale register, the same for both operands (read by no other form)
  [[maybe_unused]] const int mx_scale = kFp4ScaleWord;
  // one stage of SC columns; fresh = first stage of a fold group (the chains
  // restart; never with deferred folds, whose chains are zeroed at the fold
  // instead).  B fragments go through two register sets: k-step i+1's are
  // read while k-step i's 16 MFMAs issue.
  // (ct0, ct1: the stage's column tiles of this call -- the wide form runs a
  // stage in two calls, see the pair loop; the last fragment read by the first
  // waits in bh for the second)
  f16x8 bh[2];
  auto compute = [&](int buf, bool fresh_stage, int ct0 = 0, int ct1 = C::NCT) {
    // (deferred folds: the chains occupy their registers over the whole pair
    // loop, so the B offsets are formed anew from the lane id here instead of
    // being kept across it -- see fresh_lane())
    [[maybe_unused]] int bb = 0, bs = 0;
    if constexpr (kDefer) {
      const int fl = static_cast<int>(fresh_lane()), fli = fl & 15, flq = fl >> 4;
      bb = fli * C::SLOTS + (flq ^ (C::swz(fli) & 3));
      bs = C::swz(fli) & ~3;
    }
    auto load_b = [&](int set, int c, int ct) {
      if constexpr (kDefer)
        bh[set] = __builtin_bit_cast(f16x8, lds[buf * C::F4 + ct * 16 * C::SLOTS + bb + ((c * C::LG) ^ bs)]);
      else
        bh[set] = __builtin_bit_cast(f16x8, lds[buf * C::F4 + ct * 16 * C::SLOTS + b_off(c)]);
    };
    if (ct0 == 0) load_b(0, 0, 0);
#pragma unroll
    for (int ct = ct0; ct < ct1; ++ct) {
      __builtin_amdgcn_sched_barrier(0);
      const bool fresh = fresh_stage && ct == 0;
#pragma unroll
      for (int c = 0; c < C::NKS; ++c) {
        constexpr int KPC = C::NKS / C::NCH;  // k-steps per chain
        const int ch = c / KPC;
        const int i = ct * C::NKS + c, cur = i & 1;
        if (c + 1 < C::NKS)
          load_b(cur ^ 1, c + 1, ct);
        else if (ct + 1 < C::NCT)
          load_b(cur ^ 1, 0, ct + 1);
        const typename C::acc4 zero = {};
#pragma unroll
        for (int rt = 0; rt < C::RT; ++rt)
          mc[ch][rt] = C::mfma(bh[cur], ah[rt][c], (c % KPC == 0 && fresh) ? zero : mc[ch][rt], mx_scale);
      }
      constexpr int NM = C::RT;  // MFMAs per k-step
#pragma unroll
      for (int c = 0; c < C::NKS; ++c) {
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // next k-step's B
        __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);  // MFMA
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // chains -> LDS row accumulator (exact integer adds: fp64, or int64 for the
  // int8 form's int32 chains and the fp4 form's fp32 chains of integers,
  // converted in Cfg::lane_sum -- Cfg::row_add).  The column tile
  // is the MFMA's M side, so lane (li, lq) holds row li of the row tile at the
  // tile's columns 4 lq .. 4 lq + 3: the 16 columns of a row are summed in the
  // lane, (m0 + m1) + (m2 + m3), and over the four lane rows, (x0 + x2) + (x1 +
  // x3), by a two-step reduce-scatter of eight tiles' sums that leaves each
  // lane 2 fully summed rows, added by all 64 lanes at distinct LDS addresses
  // (round 11; before, the rows were the M side and the 16 columns one DPP
  // row: 30 DPP adds and 60 selects per 8 tiles, 2.5 % of the launch).
  // Every chain is reduced and rounded on its own, eight row tiles at a time
  // (the wide form's 16 tiles in two rounds), so a row's integer does not
  // depend on which form held its chain.
  auto fold_rows = [&]() {
    [[maybe_unused]] int fli = 0, flq = 0;
    if constexpr (kDefer) {  // (as in compute())
      const int fl = static_cast<int>(fresh_lane());
      fli = fl & 15;
      flq = fl >> 4;
    }
#pragma unroll
    for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
      for (int t0 = 0; t0 < C::RT; t0 += 8) {
        typename C::sum_t x[8];
#pragma unroll
        for (int rt = 0; rt < 8; ++rt) {
          const typename C::acc4 m = mc[ch][t0 + rt];
          x[rt] = C::lane_sum(m);
        }
        // lanes 0-31 keep tiles 0-3, lanes 32-63 tiles 4-7; then even rows keep k, odd rows k + 2
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = swap_add<true>(x[k], x[k + 4]);
#pragma unroll
        for (int k = 0; k < 2; ++k) x[k] = swap_add<false>(x[k], x[k + 2]);
        const int row = kDefer ? wave * C::RPW + (t0 + 2 * (flq & 1) + 4 * (flq >> 1)) * 16 + fli
                               : wave * C::RPW + (t0 + 2 * (lq & 1) + 4 * (lq >> 1)) * 16 + li;
        C::row_add(&rowacc[row], x[0]);
        C::row_add(&rowacc[row + 16], x[1]);
      }
  };
  // The integer forms' chains run over up to C::FOLD_PAIRS pairs of a row unit
  // (round 15): no stage restarts them; they are zero before the first pair
  // and after every fold, and `pending` (wave-uniform) counts the pairs they
  // hold.  One compute() serves every pair -- the fp16 forms keep fresh stages
  // and the fold at the end of each pair.
  static_assert(!kDefer || (C::WIDE && C::SPP == 1 && DAL_GRAM_STAGGER > 0), "deferred folds: the wide form's pair loop");
  [[maybe_unused]] int pending = 0;
  [[maybe_unused]] auto zero_chains = [&]() {
    const typename C::acc4 zero = {};
#pragma unroll
    for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
      for (int rt = 0; rt < C::RT; ++rt) mc[ch][rt] = zero;
  };
  if constexpr (kDefer) zero_chains();
  auto flush_one = [&](typename C::racc_t& slot, int64_t out_row) {
    const typename C::racc_t v = slot;
    if (v != 0) atomicAdd(acc_out + out_row, static_cast<unsigned long long>(static_cast<long long>(v)));
    slot = 0;
  };
  auto flush_rows = [&](int ru) {  // rowacc[h * 512 + r] -> row r of the unit's super block h
    for (int e = tid; e < HV * kSB; e += C::NT) {
      const int P = sched.rowP(ru, e / kSB);
      if (sched.live(P)) flush_one(rowacc[e], static_cast<int64_t>(P) * kSB + e % kSB);
    }
  };
  // every barrier waits for this wave's LDS adds and DMA first (hipcc may
  // omit the lgkmcnt wait at a loop-top barrier after no-return LDS adds)
  auto block_sync = [&]() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
  };
  auto stage_sync = [&]() { block_sync(); };

  // Units.  The block enters unit g; every later one comes from the launch's
  // counter (claim_slot >= 0: G + the counter's value, so the blocks take the
  // remaining units in the order they finish -- a block's speed decides its
  // share, and the launch ends within one unit of the last block), or from
  // the fixed deal (claim_slot < 0: the contiguous form, no unit beyond the
  // blocks' first, or no free counter).
  // A claim is one lane's agent-scope add; its value reaches the block through
  // claim_lds at the next barrier.  Two words take the claims in turn: between
  // the block's reads of a word and lane 0's next write to it lies the barrier
  // of the claim between them.  The counter words are touched by agent-scope
  // atomics only (no other data is handed between blocks), so no fence is
  // needed.
  GramClaimCursor<HV> cur(sched, n_slices * C::NSUB);  // (the wide form's units count sub-slices)
  const bool dyn = claim_slot >= 0;
  int claim_par = 0;  // word of claim_lds of the next claim
  auto claim_begin = [&]() {
    if (dyn && tid == 0)
      claim_lds[claim_par] =
          G + static_cast<int>(__hip_atomic_fetch_add(&g_claim[claim_slot].next, 1u, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT));
  };
  auto claim_end = [&](int last) {  // last: the unit handed over before; (behind a barrier after claim_begin)
    const int u = dyn ? __builtin_amdgcn_readfirstlane(claim_lds[claim_par]) : cur.static_next(last);
    claim_par ^= 1;
    return u;
  };
  // hand the cursor the claim begun before the last barrier; a unit without a
  // pair is skipped by claiming again
  auto claim_take = [&]() {
    while (!cur.claimed(claim_end(cur.v_next))) {
      claim_begin();
      if (dyn) block_sync();
    }
  };
  // The last block to leave (every claim of the launch has returned by then)
  // zeroes the counter: the next launch that uses the slot finds it ready, in
  // stream order and under graph replay, without a memset.
  auto leave = [&]() {
    if (dyn && tid == 0) {
      const unsigned before =
          __hip_atomic_fetch_add(&g_claim[claim_slot].done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (before + 1 == static_cast<unsigned>(G)) {
        __hip_atomic_store(&g_claim[claim_slot].next, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&g_claim[claim_slot].done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  };
  if (!cur.claimed(cur.first_unit())) {  // (unit g is empty)
    claim_begin();
    if (dyn) block_sync();
    claim_take();
  }
  if (!cur.start()) {
    leave();
    return;
  }
  issue(0, cur.J, 0, cur.slice);
  load_a(cur.ru, cur.slice);
  claim_begin();  // read behind the next barrier, as after every advance() into a new unit
  int buf = 0;       // LDS stage buffer of the next stage to compute
  int flushRU = -1;  // row unit whose sums wait in rowacc

  while (true) {
    // this wave's super block takes J?  (a half whose super block does not idles)
    const bool act = cur.acts(half);

#pragma unroll
    for (int s = 0; s < C::SPP; ++s) {
      stage_sync();
      if constexpr (C::WIDE && DAL_GRAM_STAGGER > 0) {
        // The wide form's look-ahead (the claim, peek() and the next stage's
        // DMA issue: ~165 scalar instructions, ~1,300 cycles when both waves
        // of a SIMD run them at once behind the barrier with the matrix pipe
        // empty -- stamped, round 12) sits at two places of the pair: waves
        // 0-3 run it behind the barrier, their SIMD partners 4-7 behind their
        // first DAL_GRAM_STAGGER column tiles, so each runs under the other's
        // MFMAs.  Nothing of it is read by the pair's own MFMAs; the DMA goes
        // to the buffer every wave left before the barrier, the claim word
        // read here is next written two claims on, and the rare barriers in
        // claim_take() are the same in number for every wave.  The flush needs
        // only the unit noted at the last change of rows and stays behind the
        // barrier in every wave.
        if (flushRU >= 0) {
          flush_rows(flushRU);
          flushRU = -1;
        }
        auto look_ahead = [&]() {
          if (cur.new_unit) claim_take();
          cur.peek();
          if (cur.has_next) issue(buf ^ 1, cur.next_J, 0, cur.next_slice());
        };
        const bool lead = lookahead_tiles(wave, C::WAVES, DAL_GRAM_STAGGER) == 0;  // (gram_schedule.hpp)
        if (!act) {
          look_ahead();
        } else {
          if (lead) look_ahead();
          compute(buf, !kDefer, 0, DAL_GRAM_STAGGER);
          if (!lead) look_ahead();
          compute(buf, !kDefer, DAL_GRAM_STAGGER, C::NCT);
          if constexpr (kDefer)
            ++pending;
          else
            fold_rows();
        }
        if constexpr (kDefer) {
          // (every wave is past its look-ahead: rows_change is the announced pair's)
          if (fold_due(pending, C::FOLD_PAIRS, cur.rows_change)) {  // (gram_schedule.hpp)
            fold_rows();
            zero_chains();
            pending = 0;
          }
        }
        buf ^= 1;
        continue;
      }
      if (s == 0) {
        if (cur.new_unit) claim_take();
        cur.peek();
        if (flushRU >= 0) {
          flush_rows(flushRU);
          flushRU = -1;
        }
      }
      if (s + 1 < C::SPP) {
        issue(buf ^ 1, cur.J, s + 1, cur.slice);
      } else if (cur.has_next) {
        issue(buf ^ 1, cur.next_J, 0, cur.next_slice());
      }
      if (act) {  // (wave-uniform)
        compute(buf, s % C::SPF == 0);
        if (s % C::SPF == C::SPF - 1) fold_rows();
      }
      buf ^= 1;
    }

    if (cur.rows_change) flushRU = cur.ru;
    if (!cur.has_next) break;
    if (cur.advance()) load_a(cur.ru, cur.slice);
    if (cur.new_unit) claim_begin();
  }
  block_sync();
  if (flushRU >= 0) flush_rows(flushRU);
  leave();
