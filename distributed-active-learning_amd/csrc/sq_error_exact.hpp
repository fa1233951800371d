// The squared error of one row and its place in the exact accumulator of
// rf_exact_sum.hpp (sq_error.hip):
//   e = fl(y - pred), s = fl(e * e)   two roundings, no FMA,
// and of a finite nonzero s the exponent of its lowest set bit (low) and the
// exponent above its highest set bit (top): over a vector, q = min low is the
// quantum of the exact sum and top_max - q its span in bits
// (dal.random_forest.exact_sum_format).
//
// Plain C++ (no HIP call): the same code runs in the kernels and in the host
// test driver (tests/host/sq_error_driver.cpp).
#pragma once

#include <limits.h>

#include "rf_exact_sum.hpp"

namespace dal {
namespace sqerr {

constexpr int32_t kNoLow = INT32_MAX;
constexpr int32_t kNoTop = INT32_MIN;

DAL_EXACT_HD double squared_error(double pred, double y) {
#if defined(__HIP_DEVICE_COMPILE__)
  const double e = __dsub_rn(y, pred);
  return __dmul_rn(e, e);
#else
  volatile double e = y - pred;  // (volatile: each operation rounds on its own)
  volatile double s = e * e;
  return s;
#endif
}

DAL_EXACT_HD bool finite_f64(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return ((b >> 52) & 0x7FF) != 0x7FF;
}

// low and top of one nonzero value (mant != 0).
DAL_EXACT_HD int low_exponent(const exact::Parts& p) { return p.e2 + __builtin_ctzll(p.mant); }
DAL_EXACT_HD int top_exponent(const exact::Parts& p) { return p.e2 + 64 - __builtin_clzll(p.mant); }

}  // namespace sqerr
}  // namespace dal
