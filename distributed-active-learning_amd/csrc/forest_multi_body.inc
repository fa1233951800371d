// The body of the row-major multiclass kernels (forest_multi.hip), included
// into forest_multi_kernel<CW, X_LDS, F_LDS, PERSIST, DW, POW> and, with the
// step hooks, forest_multi_step_kernel<CW, X_LDS, F_LDS, PERSIST, POW>: one
// text, two kernels (a __device__ function called from both compiled the
// kernels without hooks to other instructions than they had).  In scope: CW,
// X_LDS, F_LDS, PERSIST, DW, POW, STEP and the kernel's parameters A, R, tpr,
// x_floats, vec4, pad4, dma, n_tiles.
//
// STEP (with DW; A is a McStepArgs; dal_dw_step_multiclass on a pool without a
// blocked copy): the status and flag hooks of ForestStepHooks -- the first
// thread of the grid zeroes hooks.status_reset, and the row leader's flags come
// from step_row_flag.  There is no group fold here: the step takes its
// group_min_kernel pass after this kernel.
  static_assert(!PERSIST || X_LDS, "the persistent form stages rows by LDS-DMA");
  static_assert(!STEP || DW, "the step hooks belong to the density-weighted form");
  if constexpr (STEP) {
    if (A.hooks.status_reset && blockIdx.x == 0 && threadIdx.x == 0) *A.hooks.status_reset = 0;
  }
  if (PERSIST) {
    dma = true;
    vec4 = false;
    pad4 = true;
  }
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* xs = reinterpret_cast<float*>(smem);
  double* lut_s = reinterpret_cast<double*>(smem + static_cast<size_t>(x_floats) * 4);  // (x_floats % 4 == 0)
  const int n_inner = (1 << A.depth) - 1;
  const int n_leaf = 1 << A.depth;
  const int2* inner = A.inner;
  const uint8_t* leaf = A.leaf;
  const int tid = threadIdx.x;
  for (int i = tid; i <= A.n_trees; i += kMcThreads) lut_s[i] = A.lut[i];  // (read after the staging barrier)
  if (F_LDS) {
    int2* fs = reinterpret_cast<int2*>(lut_s + round_up(A.n_trees + 1, 2));
    uint8_t* ls = reinterpret_cast<uint8_t*>(fs + A.n_trees * n_inner);
    for (int e = tid; e < A.n_trees * n_inner; e += kMcThreads) fs[e] = A.inner[e];
    for (int e = tid; e < A.n_trees * n_leaf; e += kMcThreads) ls[e] = A.leaf[e];
    inner = fs;
    leaf = ls;
  }
  // row stride in LDS: d + 1 words for scalar staging; d + 4 with 16-B staging
  // (rows stay 16-B aligned, rows of a wave start 4 banks apart)
  const int xstride = A.d + (pad4 ? 4 : 1);
  const int r = tid / tpr;  // (the row / tree-phase mapping of score_tile_multi)
  const int sub = tid - r * tpr;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {  // block-uniform
    const int64_t row0 = tile * R;
    const int64_t row = row0 + r;
    const bool live = r < R && row < A.n;
    // the row leader's flags are loaded with the tile (one HBM latency per tile)
    uint8_t fl_pre = DAL_ROW_CANDIDATE;
    if constexpr (STEP) {
      if (live && sub == 0) fl_pre = step_row_flag(A.hooks, A.flags, row);
    } else {
      if (A.flags && live && sub == 0) fl_pre = A.flags[row];
    }
    long long dens_pre = 0;  // ... and, DW, its density word
    if constexpr (DW) {
      if (live && sub == 0) dens_pre = static_cast<const long long*>(A.density)[row];
    }
    if (X_LDS) {
      const int rows_here = static_cast<int>(min(static_cast<int64_t>(R), A.n - row0));
      if (dma) {
        // LDS-DMA staging (d % 4 == 0, 16-B-aligned padded rows): one
        // global_load_lds_dwordx4 per 1 KiB of a row (the last piece with only
        // the lanes it needs), lane l's 16 B landing at M0 + 16 l
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        const int row_bytes = A.d * 4;
        for (int rr = wave; rr < rows_here; rr += kMcThreads / 64) {
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
        for (int e0 = 0; e0 < total; e0 += kMcThreads * kStageBatch) {
          typedef float v4f __attribute__((ext_vector_type(4)));
          v4f v[kStageBatch];
#pragma unroll
          for (int j = 0; j < kStageBatch; ++j) {
            const int e = e0 + j * kMcThreads + tid;
            if (e < total) {
              const int rr = e / q, c = e - rr * q;
              v[j] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(A.x + (row0 + rr) * A.ldx) + c);
            }
          }
#pragma unroll
          for (int j = 0; j < kStageBatch; ++j) {
            const int e = e0 + j * kMcThreads + tid;
            if (e < total) {
              const int rr = e / q, c = e - rr * q;
              *reinterpret_cast<v4f*>(xs + rr * xstride + 4 * c) = v[j];  // (vec4 implies pad4: 16-B aligned rows)
            }
          }
        }
      } else {
        for (int e = tid; e < rows_here * A.d; e += kMcThreads) {
          const int rr = e / A.d, c = e - rr * A.d;
          xs[rr * xstride + c] = A.x[(row0 + rr) * A.ldx + c];
        }
      }
    }
    __syncthreads();
    score_tile_multi<CW, X_LDS, DW, POW>(A, xs, xstride, tile, R, tpr, inner, leaf, fl_pre, dens_pre, lut_s);
    if (!PERSIST) break;
    __syncthreads();  // every wave done with the tile before the next one is staged
  }
