// Rate probe for the density Gram's matrix instruction: bare loops of
// v_mfma_f32_16x16x32_f16 (the wide form's) and of v_mfma_i32_16x16x64_i8 in
// the wide form's shape -- 8 waves per block, one block per CU (two waves per
// SIMD), 128 A registers per wave (16 row tiles), every B fragment re-read
// from a 32 KiB LDS stage by ds_read_b128 and used by 16 MFMAs, 512 MFMAs per
// wave and stage, the chains restarted at every stage.  No DMA, no fold, no
// barrier inside the loop.  The operands come from the caller (the pool's H
// and its int8 quantisation): the clock the chip holds depends on the data.
//
// Wave 0 of every block stamps s_memtime / s_memrealtime around its loop
// (this probe only; the product kernels carry no stamp): cycles per MFMA and
// the in-kernel clock = d(memtime) / d(memrealtime) x 100 MHz.
//
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC scripts/mfma_rate_probe.hip -o scripts/libmfma_rate_probe.so
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstring>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 8, kRT = 16, kNCT = 16, kNKS = 2;
constexpr int kStageF4 = 32768 / 16;
constexpr int kRowsPerBlock = kWaves * kRT * 16;  // 2,048 A rows
constexpr int kMfmaPerStage = kNCT * kNKS * kRT;  // 512 per wave

template <bool kI8>
struct Op;
template <>
struct Op<false> {
  using frag = f16x8;
  using acc = f32x4;
  static constexpr int kElem = 2, kFeat = 64;  // bytes per element, features per staged row (128 B)
  static __device__ __forceinline__ acc mfma(frag a, frag b, acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Op<true> {
  using frag = i32x4;
  using acc = i32x4;
  static constexpr int kElem = 1, kFeat = 128;
  static __device__ __forceinline__ acc mfma(frag a, frag b, acc c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
  }
};

// ops: [n_rows][ld bytes] operand rows (fp16 H or int8 a), n_rows a power of two
// >= 2,048; stamps: [grid][4] = memtime, memrealtime before and after the loop.
template <bool kI8>
__global__ __launch_bounds__(64 * kWaves, 1) void rate_kernel(const char* __restrict__ ops, int n_rows, int ld,
                                                              int iters, unsigned long long* __restrict__ stamps,
                                                              int* __restrict__ sink) {
  using O = Op<kI8>;
  __shared__ __attribute__((aligned(16))) float4 lds[kStageF4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
  const int mask = n_rows - 1;
  // stage: 256 columns x 128 B, slot s of row R at position s ^ (R & 7)
  for (int e = tid; e < kStageF4; e += 64 * kWaves) {
    const int row = e >> 3, slot = e & 7;
    const char* src = ops + static_cast<int64_t>((blockIdx.x * 256 + row) & mask) * ld + slot * 16;
    lds[row * 8 + (slot ^ (row & 7))] = *reinterpret_cast<const float4*>(src);
  }
  typename O::frag a[kRT][kNKS];
#pragma unroll
  for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
    for (int c = 0; c < kNKS; ++c) {
      const int row = (blockIdx.x * kRowsPerBlock + wave * kRT * 16 + rt * 16 + li) & mask;
      a[rt][c] = *reinterpret_cast<const typename O::frag*>(ops + static_cast<int64_t>(row) * ld + (c * 4 + lq) * 16);
    }
  __syncthreads();
  typename O::acc mc[kRT];
  typename O::acc keep = {};
  const int b_base = li * 8 + (lq ^ (li & 3)), b_swz = li & 4;
  unsigned long long t0 = 0, r0 = 0;
  if (lane == 0 && wave == 0) {
    t0 = __builtin_amdgcn_s_memtime();
    r0 = __builtin_amdgcn_s_memrealtime();
  }
  for (int it = 0; it < iters; ++it) {
    typename O::frag b[2];
    b[0] = __builtin_bit_cast(typename O::frag, lds[b_base + (0 ^ b_swz)]);
#pragma unroll
    for (int ct = 0; ct < kNCT; ++ct) {
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < kNKS; ++c) {
        const int i = ct * kNKS + c, cur = i & 1;
        const int nct = c + 1 < kNKS ? ct : ct + 1, nc = c + 1 < kNKS ? c + 1 : 0;
        if (nct < kNCT) b[cur ^ 1] = __builtin_bit_cast(typename O::frag, lds[nct * 128 + b_base + ((nc * 4) ^ b_swz)]);
        const typename O::acc zero = {};
#pragma unroll
        for (int rt = 0; rt < kRT; ++rt) mc[rt] = O::mfma(b[cur], a[rt][c], (ct == 0 && c == 0) ? zero : mc[rt]);
      }
#pragma unroll
      for (int c = 0; c < kNKS; ++c) {
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, kRT, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // keep every chain live without a fold: one xor per chain and stage
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt) {
      const i32x4 v = __builtin_bit_cast(i32x4, mc[rt]);
      i32x4 k = __builtin_bit_cast(i32x4, keep);
      k[rt & 3] ^= v[rt & 3];
      keep = __builtin_bit_cast(typename O::acc, k);
    }
  }
  if (lane == 0 && wave == 0) {
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    unsigned long long* s = stamps + 4 * blockIdx.x;
    s[0] = t0;
    s[1] = r0;
    s[2] = t1;
    s[3] = r1;
  }
  const i32x4 k = __builtin_bit_cast(i32x4, keep);
  if ((k[0] ^ k[1] ^ k[2] ^ k[3]) == 0x5eed5eed) sink[0] = 1;  // (never: keeps the chains)
}

// ops_h: host operand [n_rows][ld bytes]; runs back-to-back launches for
// warm_s seconds, then `timed` launches between events.  out: [0] ms per timed
// launch, [1] MFMAs per wave per launch, [2] grid; stamps_h: [grid][4] of the
// last launch.
extern "C" int mfma_rate(int i8, const void* ops_h, int n_rows, int ld, int iters, double warm_s, int timed,
                         double* out, unsigned long long* stamps_h, int max_grid) {
  if (n_rows < kRowsPerBlock || (n_rows & (n_rows - 1)) || ld < 128 || ld % 16) return 2;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
  const int grid = prop.multiProcessorCount < max_grid ? prop.multiProcessorCount : max_grid;
  char* ops;
  unsigned long long* stamps;
  int* sink;
  const size_t bytes = static_cast<size_t>(n_rows) * ld;
  if (hipMalloc(&ops, bytes) || hipMalloc(&stamps, 32 * grid) || hipMalloc(&sink, 4)) return 1;
  hipMemcpy(ops, ops_h, bytes, hipMemcpyHostToDevice);
  hipMemset(sink, 0, 4);
  auto launch = [&]() {
    if (i8)
      hipLaunchKernelGGL(rate_kernel<true>, dim3(grid), dim3(64 * kWaves), 0, 0, ops, n_rows, ld, iters, stamps, sink);
    else
      hipLaunchKernelGGL(rate_kernel<false>, dim3(grid), dim3(64 * kWaves), 0, 0, ops, n_rows, ld, iters, stamps, sink);
  };
  const auto w0 = std::chrono::steady_clock::now();
  while (std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() < warm_s) {
    for (int i = 0; i < 8; ++i) launch();
    if (hipDeviceSynchronize() != hipSuccess) return 3;
  }
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipEventRecord(e0, 0);
  for (int i = 0; i < timed; ++i) launch();
  hipEventRecord(e1, 0);
  if (hipEventSynchronize(e1) != hipSuccess) return 3;
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  out[0] = ms / timed;
  out[1] = static_cast<double>(iters) * kMfmaPerStage;
  out[2] = grid;
  const int rc = hipMemcpy(stamps_h, stamps, 32 * grid, hipMemcpyDeviceToHost) != hipSuccess;
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  hipFree(ops);
  hipFree(stamps);
  hipFree(sink);
  return rc;
}
