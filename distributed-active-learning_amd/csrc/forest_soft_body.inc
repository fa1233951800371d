// The body of the soft-vote kernels (forest_soft.hip), included into
// forest_soft_kernel<W, X_LDS, F_LDS, PERSIST> and the density-weighted
// forest_soft_dw_kernel<W, X_LDS, F_LDS, PERSIST, POW>: one text, two kernels
// (the way forest_multi_body.inc serves the hard-vote kernels; the uncertainty
// kernel keeps its name, its argument struct and its instructions).  In scope:
// W, X_LDS, F_LDS, PERSIST, DW, POW, BALD and the kernel's parameters A, R,
// tpr, x_floats, vec4, pad4, dma, n_tiles.
//
// DW (A is a SoftDwArgs): the row leader's density word is loaded with its
// flags, once per tile; the first thread of the grid zeroes A.status_reset
// (dal_dw_step_soft's DAL_STEP_RESET_STATUS).
//
// BALD (A is a SoftBaldArgs): a leaf's LDS row is round2(C + 1) words, the
// entropy word A.leaf_h[l] at column C.
  static_assert(!PERSIST || X_LDS, "the persistent form stages rows by LDS-DMA");
  soft_reset_status<DW>(A);
  if (PERSIST) {
    dma = true;
    vec4 = false;
    pad4 = true;
  }
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* xs = reinterpret_cast<float*>(smem);
  const int n_inner = (1 << A.depth) - 1;
  const int n_leaf = 1 << A.depth;
  const int2* inner = A.inner;
  const int32_t* leaf_id = A.leaf_id;
  const uint32_t* leaf_q = A.leaf_q;
  int qstride = A.n_classes;
  const int tid = threadIdx.x;
  if (F_LDS) {
    // (x_floats % 4 == 0: the nodes start 16-B aligned)
    int2* fs = reinterpret_cast<int2*>(smem + static_cast<size_t>(x_floats) * 4);
    int32_t* ls = reinterpret_cast<int32_t*>(fs + A.n_trees * n_inner);
    const size_t q_off = static_cast<size_t>(
        round_up(static_cast<int64_t>(x_floats) * 4 + static_cast<int64_t>(A.n_trees) * (n_inner * 8 + n_leaf * 4), 16));
    uint32_t* qs = reinterpret_cast<uint32_t*>(smem + q_off);
    qstride = soft_lds_row<BALD>(A.n_classes);
    for (int e = tid; e < A.n_trees * n_inner; e += kSoftThreads) fs[e] = A.inner[e];
    for (int e = tid; e < A.n_trees * n_leaf; e += kSoftThreads) ls[e] = A.leaf_id[e];
    for (int e = tid; e < A.n_leaves * qstride; e += kSoftThreads) {
      const int l = e / qstride, c = e - l * qstride;
      qs[e] = soft_lds_word<BALD>(A, l, c);
    }
    inner = fs;
    leaf_id = ls;
    leaf_q = qs;
  }
  // row stride in LDS: d + 1 words for scalar staging; d + 4 with 16-B staging
  // (rows stay 16-B aligned, rows of a wave start 4 banks apart)
  const int xstride = A.d + (pad4 ? 4 : 1);
  const int r = tid / tpr;  // (the row / tree-phase mapping of score_tile_soft)
  const int sub = tid - r * tpr;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // block-uniform
    const int64_t row0 = tile * R;
    const int64_t row = row0 + r;
    const bool live = r < R && row < A.n;
    // the row leader's flags are loaded with the tile (one HBM latency per tile)
    uint8_t fl_pre = DAL_ROW_CANDIDATE;
    if (A.flags && live && sub == 0) fl_pre = A.flags[row];
    long long dens_pre = 0;  // ... and, DW, its density word
    if (DW && live && sub == 0) dens_pre = soft_density_word<DW>(A, row);
    if (X_LDS) {
      const int rows_here = static_cast<int>(min(static_cast<int64_t>(R), A.n - row0));
      if (dma) {
        // LDS-DMA staging (d % 4 == 0, 16-B-aligned padded rows): one
        // global_load_lds_dwordx4 per 1 KiB of a row (the last piece with only
        // the lanes it needs), lane l's 16 B landing at M0 + 16 l
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        const int row_bytes = A.d * 4;
        for (int rr = wave; rr < rows_here; rr += kSoftThreads / 64) {
          const float* src = A.x + (row0 + rr) * A.ldx;
          for (int p = 0; p * 1024 < row_bytes; ++p) {
            typedef __attribute__((address_space(3))) float lds_float;
            const unsigned dst = __builtin_amdgcn_readfirstlane(
                static_cast<unsigned>(reinterpret_cast<uintptr_t>((lds_float*)(xs + rr * xstride + p * 256))));
            const unsigned voff = static_cast<unsigned>(p * 1024 + lane * 16);
            if (static_cast<int>(voff) < row_bytes) lds_dma_x4(voff, dst, src);
          }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else if (vec4) {
        // 16-B loads, kStageBatch per thread issued before any LDS write
        constexpr int kStageBatch = 8;
        const int q = A.d >> 2, total = rows_here * q;
        for (int e0 = 0; e0 < total; e0 += kSoftThreads * kStageBatch) {
          typedef float v4f __attribute__((ext_vector_type(4)));
          v4f v[kStageBatch];
#pragma unroll
          for (int j = 0; j < kStageBatch; ++j) {
            const int e = e0 + j * kSoftThreads + tid;
            if (e < total) {
              const int rr = e / q, c = e - rr * q;
              v[j] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(A.x + (row0 + rr) * A.ldx) + c);
            }
          }
#pragma unroll
          for (int j = 0; j < kStageBatch; ++j) {
            const int e = e0 + j * kSoftThreads + tid;
            if (e < total) {
              const int rr = e / q, c = e - rr * q;
              *reinterpret_cast<v4f*>(xs + rr * xstride + 4 * c) = v[j];  // (vec4 implies pad4: 16-B aligned rows)
            }
          }
        }
      } else {
        for (int e = tid; e < rows_here * A.d; e += kSoftThreads) {
          const int rr = e / A.d, c = e - rr * A.d;
          xs[rr * xstride + c] = A.x[(row0 + rr) * A.ldx + c];
        }
      }
    }
    __syncthreads();
    score_tile_soft<W, X_LDS, F_LDS, DW, POW, BALD>(A, xs, xstride, tile, R, tpr, inner, leaf_id, leaf_q, qstride,
                                                    fl_pre, dens_pre, soft_leaf_h<BALD>(A));
    if (!PERSIST) break;
    __syncthreads();  // every wave done with the tile before the next one is staged
  }
