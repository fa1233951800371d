// Exact, order-free sums of integer-weighted fp64 values: the accumulator of
// the regression trainer's variance histograms (rf_train_regress.hip).
//
// A vector of finite doubles is described on the host by a quantum exponent Q
// (the lowest set bit over its nonzero values, so every value is an integer
// multiple of 2^Q) and a limb count K.  A value y becomes K signed limbs
//   y / 2^Q = sign(y) * sum_j digit_j * 2^(31 j),  0 <= digit_j < 2^31,
//   limb_j = sign(y) * digit_j  (an int32),
// and a cell of K int64 words accumulates w * limb_j per word with integer adds
// (atomics on the device): |word_j| < 2^31 * (total weight), so a total weight
// below 2^31 cannot overflow, and integer adds commute -- the cell is the
// exact sum whatever the arrival order.  Cells add and subtract word by word.
// to_double gives RN(2^Q * sum_j word_j 2^(31 j)): one round to nearest even.
//
// Plain C++ (no HIP call): the same code runs in the kernels and in the host
// test driver (tests/host/rf_exact_sum_driver.cpp).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "dal.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DAL_EXACT_HD __host__ __device__ inline
#else
#define DAL_EXACT_HD inline
#endif

namespace dal {
namespace exact {

constexpr int kLimbBits = 31;
constexpr int kMaxLimbs = DAL_RF_REG_MAX_LIMBS;
constexpr int kWide = 5;  // 64-bit words of to_double's integer: 31 * kMaxLimbs + 31 (weights) + sign <= 320
static_assert(kLimbBits * kMaxLimbs + 32 <= 64 * kWide, "to_double's integer holds the widest cell");

// A finite double as sign * mant * 2^e2, mant < 2^53 (0 for +-0.0).
struct Parts {
  uint64_t mant;
  int e2;
  bool neg;
};

DAL_EXACT_HD Parts parts(double y) {
  uint64_t b;
  memcpy(&b, &y, 8);
  const int be = static_cast<int>((b >> 52) & 0x7FF);
  const uint64_t frac = b & ((uint64_t{1} << 52) - 1);
  Parts p;
  p.neg = (b >> 63) != 0;
  p.mant = be ? (frac | (uint64_t{1} << 52)) : frac;
  p.e2 = (be ? be : 1) - 1075;
  return p;
}

// limb j of p for the quantum 2^Q (Q <= the lowest set bit of the value).
DAL_EXACT_HD int32_t limb(const Parts& p, int Q, int j) {
  uint64_t m = p.mant;
  int shift = p.e2 - Q;  // the integer y / 2^Q is m * 2^shift
  if (shift < 0) {       // only zero bits leave: Q does not exceed the lowest set bit
    m = shift > -64 ? m >> -shift : 0;
    shift = 0;
  }
  const int lo = kLimbBits * j - shift;  // the limb is bits [lo, lo + 31) of m
  uint64_t v = 0;
  if (lo >= 0) v = lo < 64 ? m >> lo : 0;
  else if (lo > -kLimbBits) v = m << -lo;  // bits above the limb fall to the mask
  const int32_t digit = static_cast<int32_t>(v & ((uint64_t{1} << kLimbBits) - 1));
  return p.neg ? -digit : digit;
}

DAL_EXACT_HD int32_t limb(double y, int Q, int j) { return limb(parts(y), Q, j); }

// r = a + b and r = a - b over K words, each array with its own stride.
DAL_EXACT_HD void add(int64_t* r, int rs, const int64_t* a, int as, const int64_t* b, int bs, int K) {
  for (int j = 0; j < K; ++j) r[j * rs] = a[j * as] + b[j * bs];
}
DAL_EXACT_HD void sub(int64_t* r, int rs, const int64_t* a, int as, const int64_t* b, int bs, int K) {
  for (int j = 0; j < K; ++j) r[j * rs] = a[j * as] - b[j * bs];
}

// RN(2^Q * sum_{j < K} word(j) * 2^(31 j)): the words are summed into a
// 320-bit two's complement integer (carry propagation), negated when
// negative, and the top 53 bits are rounded to nearest even with everything
// below as the sticky bit.  A result in the subnormal range is rounded at
// 2^-1074; an exact zero is +0.0.  Loops are fixed-length so that the integer
// stays in registers.
template <class Word>
DAL_EXACT_HD double to_double(Word word, int K, int Q) {
  uint64_t a[kWide];
#pragma unroll
  for (int i = 0; i < kWide; ++i) a[i] = 0;
#pragma unroll
  for (int j = 0; j < kMaxLimbs; ++j) {
    if (j >= K) continue;
    const int64_t w = word(j);
    const int at = (kLimbBits * j) >> 6, sh = (kLimbBits * j) & 63;
    const uint64_t ext = w < 0 ? ~uint64_t{0} : 0;
    const uint64_t u = static_cast<uint64_t>(w);
    // w * 2^(31 j), sign-extended, as words at, at + 1, ... of the integer
    const uint64_t p0 = u << sh;
    const uint64_t p1 = sh ? ((u >> (64 - sh)) | (ext << sh)) : ext;
    unsigned carry = 0;
#pragma unroll
    for (int i = 0; i < kWide; ++i) {
      if (i < at) continue;
      const uint64_t addend = i == at ? p0 : (i == at + 1 ? p1 : ext);
      const uint64_t s = a[i] + addend;
      const unsigned c1 = s < addend;
      const uint64_t s2 = s + carry;
      const unsigned c2 = s2 < s;
      a[i] = s2;
      carry = c1 | c2;
    }
  }
  const bool neg = (a[kWide - 1] >> 63) != 0;
  if (neg) {
    unsigned carry = 1;
#pragma unroll
    for (int i = 0; i < kWide; ++i) {
      const uint64_t s = ~a[i] + carry;
      carry = (carry && s == 0) ? 1u : 0u;
      a[i] = s;
    }
  }
  int ti = -1;
#pragma unroll
  for (int i = 0; i < kWide; ++i)
    if (a[i]) ti = i;
  if (ti < 0) return 0.0;
  uint64_t hi = 0, mid = 0, below = 0;
#pragma unroll
  for (int i = 0; i < kWide; ++i) {
    if (i == ti) hi = a[i];
    else if (i == ti - 1) mid = a[i];
    else if (i < ti - 1) below |= a[i];
  }
  // magnitude = (hi:mid) * 2^base + (words below), in units of 2^Q
  int lz = 0;
  while (!((hi << lz) >> 63)) ++lz;
  const int bits = 128 - lz;             // of (hi:mid); hi != 0, so >= 65
  const int base = 64 * (ti - 1) + Q;    // exponent of mid's bit 0
  const int e_top = bits - 1 + base;
  const int e_lsb = e_top - 52 > -1074 ? e_top - 52 : -1074;
  const int s = e_lsb - base;            // in [12, 127]: Q >= -1074 for doubles
  uint64_t mant, rem_hi, rem_lo, half_hi, half_lo;
  if (s >= 64) {
    mant = hi >> (s - 64);
    rem_hi = s == 64 ? 0 : hi & ((uint64_t{1} << (s - 64)) - 1);
    rem_lo = mid;
    half_hi = s == 64 ? 0 : uint64_t{1} << (s - 65);
    half_lo = s == 64 ? uint64_t{1} << 63 : 0;
  } else {
    mant = (hi << (64 - s)) | (mid >> s);
    rem_hi = 0;
    rem_lo = mid & ((uint64_t{1} << s) - 1);
    half_hi = 0;
    half_lo = uint64_t{1} << (s - 1);
  }
  const bool above = rem_hi > half_hi || (rem_hi == half_hi && rem_lo > half_lo);
  const bool tie = rem_hi == half_hi && rem_lo == half_lo;
  if (above || (tie && (below != 0 || (mant & 1)))) ++mant;
  const double r = ldexp(static_cast<double>(mant), e_lsb);
  return neg ? -r : r;
}

}  // namespace exact
}  // namespace dal
