// The int8 form of the density Gram's MFMA operand (plain C++, host and
// device; tests/test_gram_i8_algebra.py restates it in NumPy).
//
// Every split-operand element is H + L (two fp16 terms, see gram_sym.hip).
// The int8 form writes H = 32 a + (H - 32 a) with
//   a(h) = clamp(rint(h / 32), -127, 127)     (ties to even; h / 32 is exact)
// and lets the MFMAs form sum_j <a_i, a_j> alone, in int32.  Where the fp16
// form's closed form (dal_gram_sym_residual) decodes (h, l), the int8 form's
// decodes
//   h' = 32 a(h),   l' = (h - h') + l         (exact: multiples of 2^-24 below 2^13)
// so that h' + l' = h + l and the density is completed exactly as before.
// The quality of a does not matter for that: a clamped a only makes l' larger.
#pragma once

#ifdef __HIPCC__
#define DAL_I8_HD __host__ __device__
#else
#define DAL_I8_HD
#endif

namespace dal {

constexpr float kI8Step = 32.0f;     // H units per int8 step
constexpr int kI8AccShift = 18;      // an int32 row sum s adds s << 18 to the accumulator (32 * 32 * 2^8)

// One row's int32 sum over a pair's 256 columns x 128 features, whatever the
// bytes: dal_quant_i8 writes -127..127, but the Gram entry point takes any
// operand, and a byte may be -128.  Chains that run over R pairs of one row
// unit before they are folded (round 15; Cfg::FOLD_PAIRS in gram_sym.hip) need
// R kI8RowMax < 2^31: R <= 3.  (With |a| <= 127 alone, 256 x 128 x 127^2 =
// 528,515,072, four pairs would fit; the fourth is given up for the byte -128.)
constexpr long long kI8RowMax = 256LL * 128 * 128 * 128;
constexpr int kI8FoldPairsMax = 3;
static_assert(kI8RowMax == (1LL << 29) && kI8FoldPairsMax * kI8RowMax < (1LL << 31) &&
                  (kI8FoldPairsMax + 1) * kI8RowMax >= (1LL << 31),
              "int32 row sums over R pairs");

DAL_I8_HD inline int quant_i8(float h) {
  const float q = __builtin_rintf(h * (1.0f / kI8Step));
  return static_cast<int>(q > 127.0f ? 127.0f : q >= -127.0f ? q : -127.0f);  // (a NaN: -127, a defined value)
}

// (h, l) -> (h', l') in place
DAL_I8_HD inline void requant_i8(double& h, double& l) {
  const double hq = static_cast<double>(kI8Step) * quant_i8(static_cast<float>(h));
  l = (h - hq) + l;
  h = hq;
}

}  // namespace dal
