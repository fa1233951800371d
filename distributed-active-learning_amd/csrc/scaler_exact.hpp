// Exact column moments of fp32 rows for the StandardScaler (scaler.hip): the
// fp32 side of the exact accumulator of rf_exact_sum.hpp.
//
// A finite fp32 value x is sign * m * 2^e with m < 2^24, so x is exact::Parts
// {m, e} and x*x is exact::Parts {m*m, 2e}: m*m < 2^48 fits the 53-bit
// mantissa, the square is exact.  Column c of a pool is described by
//   low_c  the minimum over its nonzero values of the lowest set bit's exponent
//   top_c  the maximum over its nonzero values of (the top bit's exponent) + 1
// (kNoLow / kNoTop for a column of zeros), from which
//   q_c = low_c               the quantum of S1 = sum x     is 2^q_c,
//                             the quantum of S2 = sum x*x   is 2^(2 q_c),
//   K1  = max_c ceil((top_c - low_c) / 31)      limbs of x   (at least 1),
//   K2  = max_c ceil(2 (top_c - low_c) / 31)    limbs of x*x (at least 1).
// A column whose squares need more than DAL_RF_REG_MAX_LIMBS limbs, that is
// top_c - low_c > kMaxSpan = 124 bits, is refused.
//
// Plain C++ (no HIP call): the same code runs in the kernels and in the host
// test driver (tests/host/scaler_exact_driver.cpp).
#pragma once

#include <limits.h>

#include "rf_exact_sum.hpp"

namespace dal {
namespace scaler {

constexpr int32_t kNoLow = INT32_MAX;
constexpr int32_t kNoTop = INT32_MIN;
constexpr int kMaxSpan = exact::kLimbBits * exact::kMaxLimbs / 2;  // 124: 2 * span <= 248 bits of x*x

// The bits of a finite fp32 value as sign * mant * 2^e2, mant < 2^24 (0 for +-0.0).
DAL_EXACT_HD exact::Parts parts_f32(uint32_t b) {
  const int be = static_cast<int>((b >> 23) & 0xFF);
  const uint32_t frac = b & ((1u << 23) - 1);
  exact::Parts p;
  p.neg = (b >> 31) != 0;
  p.mant = be ? (frac | (1u << 23)) : frac;
  p.e2 = (be ? be : 1) - 150;
  return p;
}

// The exact square of p (mant < 2^24): mant^2 < 2^48 at twice the exponent.
DAL_EXACT_HD exact::Parts square(const exact::Parts& p) {
  exact::Parts s;
  s.neg = false;
  s.mant = p.mant * p.mant;
  s.e2 = 2 * p.e2;
  return s;
}

DAL_EXACT_HD bool finite_f32(uint32_t b) { return ((b >> 23) & 0xFF) != 0xFF; }

// low and top of one nonzero value (mant != 0).
DAL_EXACT_HD int low_exponent(const exact::Parts& p) {
  return p.e2 + __builtin_ctzll(p.mant);
}
DAL_EXACT_HD int top_exponent(const exact::Parts& p) {
  return p.e2 + 64 - __builtin_clzll(p.mant);
}

DAL_EXACT_HD int limbs_for(int span) {
  const int k = (span + exact::kLimbBits - 1) / exact::kLimbBits;
  return k < 1 ? 1 : k;
}

// The limb counts of a pool from its columns' (low, top); q[c] (nullable)
// receives the column quanta (0 for a column of zeros).  Returns -1, or the
// first column whose span exceeds kMaxSpan (k1, k2 and q are then unspecified).
inline int64_t limb_counts(const int32_t* low, const int32_t* top, int64_t d, int32_t* k1, int32_t* k2,
                           int32_t* q) {
  int a = 1, b = 1;
  for (int64_t c = 0; c < d; ++c) {
    const bool zeros = low[c] == kNoLow || top[c] == kNoTop;
    if (q) q[c] = zeros ? 0 : low[c];
    if (zeros) continue;
    const int64_t span = static_cast<int64_t>(top[c]) - low[c];
    if (span < 1 || span > kMaxSpan) return c;
    const int s = static_cast<int>(span);
    if (limbs_for(s) > a) a = limbs_for(s);
    if (limbs_for(2 * s) > b) b = limbs_for(2 * s);
  }
  *k1 = a;
  *k2 = b;
  return -1;
}

}  // namespace scaler
}  // namespace dal
