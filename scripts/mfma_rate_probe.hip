// Rate probe for the density Gram's matrix instruction: bare loops of
// v_mfma_f32_16x16x32_f16 (the wide form's), of v_mfma_i32_16x16x64_i8 and of
// v_mfma_scale_f32_16x16x128_f8f6f4 with fp4 (e2m1) operands on both sides in
// the wide form's shape -- 8 waves per block, one block per CU (two waves per
// SIMD), 128 A registers per wave (16 row tiles), every B fragment re-read
// from a 32 KiB LDS stage by ds_read_b128 and used by 16 MFMAs, 512 MFMAs per
// wave and stage, the chains restarted at every stage.  No DMA, no fold, no
// barrier inside the loop.  The operands come from the caller (the pool's H,
// its int8 and its fp4 quantisation): the clock the chip holds depends on the
// data.  A staged row is 128 B in every form: 64 fp16, 128 int8 or 256 fp4
// features.
//
// mfma_fp4_exact runs the scaled instruction on chains of the Gram kernel's
// own length (16 column tiles x 2 k-steps into one accumulator) from packed
// fragments and a C input of the caller's, one wave per chain, and returns
// every accumulator element: the caller compares them with the int64 values.
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
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int kWaves = 8, kRT = 16, kNCT = 16, kNKS = 2;
constexpr int kStageF4 = 32768 / 16;
constexpr int kRowsPerBlock = kWaves * kRT * 16;  // 2,048 A rows
constexpr int kMfmaPerStage = kNCT * kNKS * kRT;  // 512 per wave

// fp4 operands, one E8M0 scale byte per lane and side (the instruction reads
// four registers of each operand at cbsz:4 blgp:4)
__device__ __forceinline__ f32x4 mfma_fp4(i32x4 a, i32x4 b, f32x4 c, int scale) {
  const i32x8 a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0}, b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, c, 4, 4, 0, scale, 0, scale);
}

constexpr int kF16 = 0, kI8 = 1, kFp4 = 2;
template <int kForm>
struct Op;
template <>
struct Op<kF16> {
  using frag = f16x8;
  using acc = f32x4;
  static __device__ __forceinline__ acc mfma(frag a, frag b, acc c, int) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Op<kI8> {
  using frag = i32x4;
  using acc = i32x4;
  static __device__ __forceinline__ acc mfma(frag a, frag b, acc c, int) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
  }
};
template <>
struct Op<kFp4> {
  using frag = i32x4;
  using acc = f32x4;
  static __device__ __forceinline__ acc mfma(frag a, frag b, acc c, int scale) { return mfma_fp4(a, b, c, scale); }
};

// ops: [n_rows][ld bytes] operand rows (fp16 H, int8 a or fp4 codes), n_rows a
// power of two >= 2,048; stamps: [grid][4] = memtime, memrealtime before and
// after the loop; scale: the fp4 form's E8M0 byte in every byte of the word.
template <int kForm>
__global__ __launch_bounds__(64 * kWaves, 1) void rate_kernel(const char* __restrict__ ops, int n_rows, int ld,
                                                              int iters, unsigned long long* __restrict__ stamps,
                                                              int* __restrict__ sink, int scale_arg) {
  using O = Op<kForm>;
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
  const int scale = scale_arg + 0 * lane;  // (a VGPR, set once before the loop)
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
        for (int rt = 0; rt < kRT; ++rt) mc[rt] = O::mfma(b[cur], a[rt][c], (ct == 0 && c == 0) ? zero : mc[rt], scale);
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
// form: 0 fp16, 1 int8, 2 fp4.
extern "C" int mfma_rate(int form, const void* ops_h, int n_rows, int ld, int iters, double warm_s, int timed,
                         double* out, unsigned long long* stamps_h, int max_grid, int scale) {
  if (form < 0 || form > 2) return 2;
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
    if (form == kFp4)
      hipLaunchKernelGGL(rate_kernel<kFp4>, dim3(grid), dim3(64 * kWaves), 0, 0, ops, n_rows, ld, iters, stamps, sink,
                         scale);
    else if (form == kI8)
      hipLaunchKernelGGL(rate_kernel<kI8>, dim3(grid), dim3(64 * kWaves), 0, 0, ops, n_rows, ld, iters, stamps, sink,
                         scale);
    else
      hipLaunchKernelGGL(rate_kernel<kF16>, dim3(grid), dim3(64 * kWaves), 0, 0, ops, n_rows, ld, iters, stamps, sink,
                         scale);
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

// One wave per chain: acc = c_in, then `steps` MFMAs acc = mfma(x[s], y[s], acc).
// x, y: [chains][steps][64 lanes] 16-byte fragments, c, out: [chains][64 lanes][4].
__global__ __launch_bounds__(64) void fp4_exact_kernel(const i32x4* __restrict__ x, const i32x4* __restrict__ y,
                                                       const f32x4* __restrict__ c, f32x4* __restrict__ out,
                                                       int steps, int scale_arg) {
  const int lane = threadIdx.x;
  const int scale = scale_arg + 0 * lane;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * steps * 64 + lane;
  f32x4 acc = c[blockIdx.x * 64 + lane];
  for (int s = 0; s < steps; ++s) acc = mfma_fp4(x[base + s * 64], y[base + s * 64], acc, scale);
  out[blockIdx.x * 64 + lane] = acc;
}

extern "C" int mfma_fp4_exact(const void* x_h, const void* y_h, const float* c_h, float* out_h, int chains, int steps,
                              int scale) {
  if (chains < 1 || steps < 1) return 2;
  const size_t fb = static_cast<size_t>(chains) * steps * 64 * 16, cb = static_cast<size_t>(chains) * 64 * 16;
  i32x4 *x, *y;
  f32x4 *c, *out;
  if (hipMalloc(&x, fb) || hipMalloc(&y, fb) || hipMalloc(&c, cb) || hipMalloc(&out, cb)) return 1;
  hipMemcpy(x, x_h, fb, hipMemcpyHostToDevice);
  hipMemcpy(y, y_h, fb, hipMemcpyHostToDevice);
  hipMemcpy(c, c_h, cb, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(fp4_exact_kernel, dim3(chains), dim3(64), 0, 0, x, y, c, out, steps, scale);
  const int rc = hipMemcpy(out_h, out, cb, hipMemcpyDeviceToHost) != hipSuccess ? 3 : 0;
  hipFree(x);
  hipFree(y);
  hipFree(c);
  hipFree(out);
  return rc;
}
