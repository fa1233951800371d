// The fp4 form of the density Gram's MFMA operand (plain C++, host and
// device; tests/test_gram_fp4_algebra.py restates it in NumPy).
//
// The step of gram_i8.hpp once more, on a coarser grid.  e2m1 magnitudes are
// {0, 0.5, 1, 1.5, 2, 3, 4, 6}; twice them is the integer grid
//   G = +-{0, 1, 2, 3, 4, 6, 8, 12}
// and every split-operand element H + L is written H = 32 a4 + (H - 32 a4) with
//   a4(h) = the element of G nearest to h / 32   (h / 32 is exact; a tie goes to
//           the smaller magnitude; beyond +-12: +-12; a NaN: 0)
// The MFMAs (v_mfma_scale_f32_16x16x128_f8f6f4, e2m1 on both sides) form sum_j
// <a4_i, a4_j> alone, and the closed form decodes
//   h' = 32 a4(h),   l' = (h - h') + l
// where the fp16 form decodes (h, l): h' + l' = h + l, so the density is
// completed exactly as before, and as there the quality of a4 does not matter
// -- a clamped a4 only makes l' larger.  The density identity is the int8
// form's with a4 for a:
//   sum_j <u~_r, u~_j> = 1024 sum_{taken pairs} <a4_r, a4_j> + <l'_r, S~>
//                        + <h'_r, S^{l'} + CH'_B>
// The unit of G is the int8 form's 32, so an integer row sum s adds s << 18 to
// the accumulator here too.
//
// Magnitudes.
//  * l'.  h and l are multiples of 2^-24 (fp16), h' a multiple of 32, so l' is
//    a multiple of 2^-24.  h' clamps at 384: a unit row's |h| <= 2^12 leaves
//    |h - h'| <= 4096 - 384 and |l| <= 2 (half an ulp of h), so |l'| < 2^12 + 2
//    -- below the 2^13 that the closed form's exact sums assume of every term
//    (an unclamped element has |h - h'| <= 64, half the widest grid step).
//  * One accumulator element of the kernel sums a column tile's 256 features 16
//    times between two folds: at most 16 x 256 x 144 = 589,824 < 2^24, whatever
//    the data, so the fp32 chains hold exact integers (kFp4ChainMax; four of
//    them, the lane's part of a row, stay below 2^24 as well).
//  * A row's int32 sum over a pair's 256 columns: at most 256 x 256 x 144
//    = 9,437,184 < 2^31 (kFp4RowMax).
#pragma once

#include "gram_i8.hpp"

#ifdef __HIPCC__
#define DAL_FP4_HD __host__ __device__
#else
#define DAL_FP4_HD
#endif

namespace dal {

constexpr float kFp4Step = 32.0f;    // H units per unit of G
constexpr int kFp4AccShift = 18;     // an integer row sum s adds s << 18 to the accumulator
constexpr int kFp4Max = 12;          // the largest magnitude of G
constexpr int kFp4ChainMax = 16 * 256 * kFp4Max * kFp4Max;  // one fp32 chain element between two folds
constexpr int kFp4RowMax = 256 * 256 * kFp4Max * kFp4Max;   // one row's int32 sum over a pair
static_assert(kFp4Step == kI8Step && kFp4AccShift == kI8AccShift, "the unit of G is the int8 form's");
static_assert(kFp4ChainMax == 589824 && 4 * kFp4ChainMax < (1 << 24),
              "fp32 chains and a lane's four columns are exact");
static_assert(kFp4RowMax == 9437184 && kFp4RowMax < (1LL << 31), "int32 row sums");
// Chains that run over R pairs of one row unit before they are folded (round
// 15; Cfg::FOLD_PAIRS in gram_sym.hip): an element is at most R kFp4ChainMax,
// whatever the codes.  With the fold's one conversion per tile the lane's four
// elements are added in fp32 first, so 4 R kFp4ChainMax must stay below 2^24:
// R <= 7.  Converting each element first needs R kFp4ChainMax < 2^24 alone (R
// <= 28), and the int32 row sum R kFp4RowMax < 2^31 is then far away as well.
// (scripts/mfma_chain_probe.py checks the instruction's adder on chains of
// these lengths and values.)
constexpr long long kFp4ExactBelow = 1LL << 24;  // every integer of smaller magnitude is an fp32
constexpr int kFp4FoldPairsMax = 7;
constexpr int kFp4FoldPairsMaxEach = 28;
static_assert(4LL * kFp4FoldPairsMax * kFp4ChainMax < kFp4ExactBelow &&
                  4LL * (kFp4FoldPairsMax + 1) * kFp4ChainMax >= kFp4ExactBelow,
              "a lane's fp32 sum of four chain elements over R pairs");
static_assert(1LL * kFp4FoldPairsMaxEach * kFp4ChainMax < kFp4ExactBelow &&
                  1LL * (kFp4FoldPairsMaxEach + 1) * kFp4ChainMax >= kFp4ExactBelow &&
                  1LL * kFp4FoldPairsMaxEach * kFp4RowMax < (1LL << 31),
              "one fp32 chain element over R pairs, and the int32 row sum");

// a4(h): the signed element of G
DAL_FP4_HD inline int quant_fp4(float h) {
  const float m = __builtin_fabsf(h) * (1.0f / kFp4Step);
  // (the midpoints of G; > sends a tie to the smaller magnitude, and a NaN, for which every test fails, to 0)
  const int g = m > 10.0f ? 12 : m > 7.0f ? 8 : m > 5.0f ? 6 : m > 3.5f ? 4 : m > 2.5f ? 3 : m > 1.5f ? 2
                 : m > 0.5f ? 1 : 0;
  return h < 0.0f ? -g : g;
}

// The 4-bit e2m1 code of an element of G: sign in bit 3, value index in bits
// 0-2 (1, 2, 3, 4 -> themselves, 6 -> 5, 8 -> 6, 12 -> 7).  0 has no sign: the
// code 8 (-0) is never written.
DAL_FP4_HD inline unsigned code_fp4(int g) {
  const unsigned m = static_cast<unsigned>(g < 0 ? -g : g);
  const unsigned idx = m <= 4u ? m : m == 6u ? 5u : m == 8u ? 6u : 7u;
  return idx | (g < 0 ? 8u : 0u);
}
DAL_FP4_HD inline int decode_fp4(unsigned code) {
  const unsigned idx = code & 7u;
  const int m = static_cast<int>(idx <= 4u ? idx : idx == 5u ? 6u : idx == 6u ? 8u : 12u);
  return code & 8u ? -m : m;
}

// (h, l) -> (h', l') in place
DAL_FP4_HD inline void requant_fp4(double& h, double& l) {
  const double hq = static_cast<double>(kFp4Step) * quant_fp4(static_cast<float>(h));
  l = (h - hq) + l;
  h = hq;
}

}  // namespace dal
