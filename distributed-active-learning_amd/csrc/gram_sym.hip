// Symmetric, compensated cosine Gram row-sum: the density d_i = sum_{j not in
// E} <u_i, u_j> of every pool row on fp16 MFMA at fp32-class accuracy, with S
// never stored.
//
// Reference: final_thesis/density_weighting.py:67-75 (U.multiply(UT) through
// IndexedRowMatrix/BlockMatrix), :95-100 (drop i,j in L0) and :157-161
// (groupByKey + sum per row); cosine_similarity.py:29-45 is the same product.
//
// Operand (dal_prep_split): every fp32 unit row at scale 2^12 as two fp16
// terms, H = fp16(2^12 u), L = fp16(2^12 u - H); u~ = H + L carries 2^12 u to
// 2^-22 relative, every product of two terms is exact in fp32 and lands in
// units of 2^-24.  Layout [n_pad][d_pad / KS][KS H | KS L].
//
// Symmetry.  Rows are grouped in 512-row super blocks.  Each unordered pair
// {P, Q} is multiplied once: P takes Q iff Q == P (diagonal), Q > P with P+Q
// even, or Q < P with P+Q odd (global indices, so the bits do not depend on
// the sharding).  The taker's rows are the A operand (register resident), Q's
// the B operand (LDS-staged); the kernel keeps the tile's ROW sums (-> P's
// rows).  The tile's column sums (-> Q's rows) are linear in P's rows,
// sum_{i in P} <H_i, H_j> = <sigma^H_P, H_j>, so they are added in closed
// form with the residual below (round 5; before, as sigma_P MFMAs and int64
// column flushes per pair).  The rule, the order in which a block walks its
// pairs and the launch's grid and column chunks are gram_schedule.hpp (plain
// C++ shared by the kernel and the launcher; tests/test_gram_schedule.py
// enumerates every block's walk on the CPU).
//
// Launches and units (round 10).  The round-robin column-chunk form runs ONE
// launch per density call: its units are (feature slice -- in the wide form
// below, 64-feature sub-slice --, column chunk, row unit), slice slowest, and a
// block takes unit g first and every later unit from a device counter
// (g_claim; GramClaimCursor in gram_schedule.hpp, walked on the CPU by
// tests/test_gram_claim_schedule.py and test_gram_schedule_wide.py), so a fast block
// takes more units and the launch ends within one unit of its last block --
// before, units were dealt u = g + k G and each slice was a launch with a tail
// of its own.  The contiguous form (small column operands) keeps its static
// shares and one launch per slice, walked through the same cursor.
//
// Compensation and column sums.  Both MFMA operands hold H only: the MFMAs
// form the fp16 Gram T_ij = <H_i, H_j> on the taken pairs, one product per
// feature pair.  Every other term of <u~_i, u~_j> is linear in the columns and
// is added exactly, in closed form, by dal_gram_sym_residual (the L.u~ terms
// since round 3, the column sums since round 5, the H.L terms -- a second MFMA
// per 32 features before -- since round 7).  With sigma^H_Q the sum of H over
// super block Q, S^L the sum of L and S~ the sum of u~ over every row (exact
// int64 in units of 2^-24), a row r of super block B receives
//   <L_r, S~> + <H_r, S^L + CH_B>,  CH_B = sum of sigma^H_P over P != B taking B
// (a parity-class prefix sum): <L_r, S~> is every L_r term, <H_r, S^L> every
// H_r.L_j term, <H_r, CH_B> the H.H column sums of the pairs other super
// blocks took.  d_i is then sum_j <u~_i, u~_j> with nothing dropped; the MFMA
// work per algorithmic product is one fp16 product on half the pairs, and
// each row's density is written only by its own rows' launches (no cross-GPU
// sum).
//
// Exactness of the row sums (as the earlier kernels): chains are folded to
// multiples of 2^-32 and added as integers (LDS fp64 below 2^53, int64
// atomics); the residual is an fp64 dot in a fixed order rounded to 2^-32.
// The density bits are identical for any grid, column split or GPU count.
//
// MI355X design: block = 4 waves x 128 rows (one super block), A fragments (8
// row tiles x KS features of H) in registers; B stages in a 2-deep LDS ring
// filled by global_load_lds_dwordx4 (source-side XOR swizzle -> conflict-free
// ds_read_b128).  One accumulator chain per 16-row tile (KS 128: per tile and
// 64-feature half) carries its row sums through the MFMAs and is folded to
// the LDS row accumulator every FOLD columns.  A stage holds the H run of each
// column's slice (the L run is not read here).  KS = 128 for d_pad % 128 == 0
// (the H-only A side frees the registers the L fragments held), else 64, or 32.
//
// The wide form (round 11; KS 128 with the round-robin schedule, the flagship
// shape): 8 waves x 256 rows, four super blocks P, P + 2, P + 4, P + 6 share
// each B stage.  The same 128 A registers hold 16 row tiles x 64 features, so
// the block walks every slice as two 64-feature sub-slices (the operand keeps
// its KS-128 layout; a staged column row is the 128 B of one half of its H
// run, the 8-slot swizzle of KS 64).  One 32 KiB stage is a whole 256-column
// pair and feeds 512 MFMAs per wave; a B fragment read feeds 16.  Against two
// super blocks per block (rounds 4-10) the staged bytes, B reads, barriers
// and DMA issue per MFMA halve.
//
// The pair boundary (round 12).  Stamped on that form (scripts/patches/
// stamp_gram_pair.patch), the matrix pipe stood empty for 2,900 of a pair's
// 19,300 cycles, all of it between the last MFMA of a pair and the first of
// the next and none inside a pair: 1,264 cycles to the barrier's release (the
// fold) and 1,300 to 2,900 behind it, the block's look-ahead -- the claim,
// peek() and the next stage's DMA issue, ~165 scalar instructions (with three
// turns of peek()'s column search ~350) run by all eight waves at once.  Two
// changes: GramSchedule::first_r finds the next taken column block in closed
// form away from the diagonal, and the look-ahead of waves 4-7 sits behind
// their first DAL_GRAM_STAGGER column tiles instead of behind the barrier
// (lookahead_tiles() in gram_schedule.hpp), so that each wave of a SIMD runs
// its scalar work under its partner's MFMAs.  The schedule, every chain and
// every fold are what they were: the bits do not change.
//
// The int8 form (round 13; gram_i8.hpp, dal_gram_rowsum_sym_i8_skip +
// dal_gram_sym_residual_i8: pools of KS-128 slices above the contiguous
// limit).  The step of rounds 5 and 7 once more, with integers: H = 32 a + (H -
// 32 a), a = clamp(rint(H / 32), -127, 127) an int8.  The MFMAs form only the
// row sums of <a_i, a_j> over the taken pairs -- v_mfma_i32_16x16x64_i8, the
// cycles of the fp16 instruction at twice the K, so a 128-feature slice of a
// pair is one pass of 512 MFMAs per wave instead of two -- and the closed
// form above, fed h' = 32 a and l' = (H - h') + L where it decodes (H, L),
// adds everything else.  int32 chains are exact: the MFMA part of the density
// is one integer whatever the grid, the column split or the GPU count.
// gram_i8sym_kernel is the wide form's body (gram_csym_body.inc) on the int8
// operand (dal_quant_i8): the same stages, swizzle, DMA pieces, B reads,
// look-ahead, claim and flush, byte for byte.
//
// The fp4 form (round 14; gram_fp4.hpp, dal_gram_rowsum_sym_fp4_skip +
// dal_gram_sym_residual_fp4: the int8 form's pools whose d_pad is a multiple
// of 256).  On the flagship pool a(H) only takes 0..15: the int8 MFMA spends
// 8-bit lanes on 4-bit numbers.  a4(H), the element of +-{0, 1, 2, 3, 4, 6, 8,
// 12} nearest to H / 32, is twice an e2m1 value, and
// v_mfma_scale_f32_16x16x128_f8f6f4 with e2m1 on both sides takes the cycles
// of the int8 instruction at twice the K.  A slice is 256 features here: its
// staged row is 128 B and a 16-byte fragment one K = 128 operand, so
// gram_fp4sym_kernel is the int8 instance byte for byte -- stages, swizzle, DMA
// pieces, B reads, 2 k-steps x 16 row tiles per column tile, 128 resident A
// registers, 512 MFMAs per wave and pair -- over half as many units.  The
// chains are fp32 holding exact integers (below 589,824 < 2^24 whatever the
// data; scripts/mfma_rate_probe.py checks the instruction's adder on chains
// of this length), converted to int32 at the fold; from there on the int8
// form's integers.  The closed form is fed h' = 32 a4, l' = (H - h') + L.
//
// The deferred fold (round 15; the int8 and fp4 forms).  Their chains hold
// exact integers with headroom, and a row unit's rows stay resident for a whole
// column chunk, so a wave folds its chains once per Cfg::FOLD_PAIRS pairs it
// acted on (fp4: 7 -- a lane's fp32 sum of four elements stays below 2^24;
// int8: 3 -- a row's int32 sum stays below 2^31 whatever the bytes, -128
// included) and when the rows change (fold_due in gram_schedule.hpp), instead
// of at the end of every pair, where the fold of waves 0-3 ran with the matrix
// pipe empty.  The chains are zeroed before the pair loop and after every fold
// and every MFMA accumulates into them; the flush, the barriers, the ring, the
// claims and the look-ahead are where they were, and the integers added to a
// row are the same: the bits do not change.  The fp16 forms' fp32 chains round;
// they fold every pair as before and compile to the same instructions.
#include <stdlib.h>

#include <mutex>
#include <type_traits>

#include "common.hpp"
#include "gram_fp4.hpp"
#include "gram_i8.hpp"
#include "gram_schedule.hpp"

namespace dal {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
#define AS3 __attribute__((address_space(3)))

constexpr int kSB = 512;       // super block rows

__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// One step of a reduce-scatter over the wave's four 16-lane rows: a and b
// exchange the halves the other keeps (v_permlane32_swap: a's lanes 32-63 with
// b's lanes 0-31; v_permlane16_swap: a's odd rows with b's even rows) and are
// added, so every lane ends with a's or b's sum over the two rows -- one swap
// and one add per two values, no select.  Inline asm: hipcc's builtins for
// the two swaps return the first register in both halves of their result
// (ROCm 7; the sum came out as a + a).  The s_nop covers the wait states
// between a VALU write of an operand, or an earlier swap, and the swap, which
// the compiler does not track through the asm.
template <bool kRows32, typename T>
__device__ __forceinline__ T swap_add(T a, T b) {
  if constexpr (kRows32)
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  else
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return a + b;
}

// Lane id recomputed at the point of use (asm volatile: never hoisted out of
// a loop), so lane-derived addresses are rematerialised instead of occupying
// VGPRs across the pair loop (a spill reload's vmcnt wait would drain the DMA).
__device__ __forceinline__ unsigned fresh_lane() {
  unsigned v;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(v));
  return v;
}

#ifndef DAL_GRAM_PRIO8
#define DAL_GRAM_PRIO8 1  // 8-wave kernels: s_setprio 1 for waves 4-7 (> 0) or 0-3 (< 0), 0: none
#endif
#ifndef DAL_GRAM_KS64_OCC
#define DAL_GRAM_KS64_OCC 4  // KS 64: 4-wave blocks per CU (3: 16 KiB stages, 100k x 64 -3.2 % vs 2; row sums only, 128 VGPRs: 4 blocks on 8 KiB stages 100k x 64 -0.7 %, 200k x 64 -0.5 % vs 3)
#endif
#ifndef DAL_GRAM_FOLD64
#define DAL_GRAM_FOLD64 256  // columns per row fold at KS <= 64
#endif
#ifndef DAL_GRAM_FOLD128
#define DAL_GRAM_FOLD128 256  // columns per row fold at KS 128 (<= 256: a fold never spans two pairs)
#endif
#ifndef DAL_GRAM_STAGE8
#define DAL_GRAM_STAGE8 32768  // bytes per LDS stage of the 8-wave kernel (65536: 2M x 256 1149.6 -> 1378.3 ms)
#endif
#ifndef DAL_GRAM_STAGGER
#define DAL_GRAM_STAGGER 4  // wide form: column tiles waves 4-7 run before their look-ahead (waves 0-3: none); 0: every wave behind the barrier
#endif
#ifndef DAL_GRAM_FOLD_PAIRS_FP4
#define DAL_GRAM_FOLD_PAIRS_FP4 7  // fp4 form: pairs of one row unit a chain takes between two folds (Cfg::FOLD_PAIRS; <= 7)
#endif
#ifndef DAL_GRAM_FOLD_PAIRS_I8
#define DAL_GRAM_FOLD_PAIRS_I8 3  // int8 form: the same (<= 3)
#endif
#ifndef DAL_GRAM_FP4_CVT_EACH
#define DAL_GRAM_FP4_CVT_EACH 0  // fp4 fold: convert each of a lane's four elements before the add (FOLD_PAIRS <= 28)
#endif
#ifndef DAL_GRAM_CHAIN_MAX
#define DAL_GRAM_CHAIN_MAX 2048  // the longest row chain dal_density_error_bound_sym_d charges
#endif
#ifndef DAL_GRAM_W8_KS64
#define DAL_GRAM_W8_KS64 0  // KS 64 in the 8-wave two-super-block form (round robin schedule only)
#endif
#ifndef DAL_GRAM_W8_OCC64
#define DAL_GRAM_W8_OCC64 1  // 8-wave KS-64 blocks per CU (128 VGPRs, 72 KiB of LDS: two fit)
#endif
#ifndef DAL_GRAM_KS32_OCC
#define DAL_GRAM_KS32_OCC 5  // KS 32: 4-wave blocks per CU (3: 16 KiB stages; >= 4: 8 KiB stages. Config 3: 2 -> 3 -> 4 blocks 3.944 -> 3.827 -> 3.745 ms; row sums only (94 VGPRs): 4 -> 5 blocks 3.430 -> 3.391 ms)
#endif
// I8 (the wide form only): the operands are the int8 quantisation a(H) of the
// split operand's H runs (gram_i8.hpp), [rows][d_pad] bytes in feature order;
// the kernel forms sum_j <a_i, a_j> in int32 by v_mfma_i32_16x16x64_i8 -- a
// whole 128-feature slice per pass of 512 MFMAs, where the fp16 form takes
// two.  Offsets stay in 2-byte units (ldh = d_pad / 2).
// FP4 (the wide form only, KS 256): the operands are the e2m1 codes of a4(H)
// (gram_fp4.hpp), [rows][d_pad / 2] bytes in feature order, two features per
// byte; v_mfma_scale_f32_16x16x128_f8f6f4 forms sum_j <a4_i, a4_j> in fp32
// chains that hold exact integers -- a whole 256-feature slice per pass of 512
// MFMAs.  ldh = d_pad / 4.
constexpr int kFormF16 = 0, kFormI8 = 1, kFormFp4 = 2;
// The fp4 form's scale word: E8M0 128 (a factor 2) in every byte, for both
// operands.  An e2m1 value is half its element of G, so with scales of 2 the
// accumulator holds sum a4 a4 itself -- an integer that v_cvt_i32_f32 takes as
// it is; unit scales (127) would leave a quarter of it and a multiply at every
// fold.  The probe found both exact.
constexpr int kFp4ScaleWord = static_cast<int>(0x80808080u);
template <int KS, int W = 4, int HVS = W / 4, int FORM = kFormF16>
struct Cfg {
  static constexpr bool I8 = FORM == kFormI8;
  static constexpr bool FP4 = FORM == kFormFp4;
  static constexpr bool INT = I8 || FP4;            // exact integer row sums, the rest in closed form
  static constexpr int WAVES = W;                   // 4: one super block per block; 8: two (P, P + 2) or four
  static constexpr int HALVES = HVS;                // super blocks per block
  // the wide form: 8 waves hold four super blocks (P, P + 2, P + 4, P + 6), 256
  // rows per wave, over sub-slices of half the slice's features -- the same
  // A registers as 128 rows x KS features, twice the rows per staged B byte
  static constexpr bool WIDE = HVS == 4;
  static constexpr int KW = WIDE && !INT ? KS / 2 : KS;  // features of the resident A fragments, of a staged row
  static constexpr int NSUB = KS / KW;              // sub-slices per slice
  static constexpr int WPS = W / HVS;               // waves per super block: 4, or 2
  static constexpr int RPW = kSB / WPS;             // rows per wave: 128, or 256
  static constexpr int NT = 64 * W;                 // threads
  // bytes per staged operand row of a sub-slice (its H run)
  static constexpr int ROWB = FP4 ? KW / 2 : KW * (I8 ? 1 : 2);
  // halves from the launch's first slice to sub-slice q: the operand keeps H run | L run per KS-slice
  static constexpr int sub_off(int q) {
    return FP4 ? q * KS / 4 : I8 ? q * KS / 2 : (q / NSUB) * 2 * KS + (q % NSUB) * KW;
  }
  static constexpr int SLOTS = ROWB / 16;           // 16-B slots per row: 4 / 8 / 16
  // three 4-wave blocks per CU at KS 64 (OCC3): 16 KiB stages so three fit the LDS
  static constexpr int OCC = W == 8 ? (KS == 64 ? DAL_GRAM_W8_OCC64 : 1)
                                    : KS == 32 ? DAL_GRAM_KS32_OCC : KS == 64 ? DAL_GRAM_KS64_OCC : 2;
  static constexpr int STAGE = W == 8 ? DAL_GRAM_STAGE8 : OCC >= 4 ? 8192 : OCC == 3 ? 16384 : 32768;  // bytes per LDS stage
  static constexpr int SC = STAGE / ROWB;           // columns per stage: 64 / 128 / 256
  static constexpr int SPP = 256 / SC;              // stages per 512 x 256 pair: 4 / 2 / 1
  static_assert(SC >= 16 && SC <= 256, "a stage holds 16 to 256 whole columns");
  static constexpr int FOLD = KS >= 128 ? DAL_GRAM_FOLD128 : DAL_GRAM_FOLD64;  // columns per row fold
  static constexpr int SPF = FOLD / SC;             // stages per fold group
  static constexpr int F4 = STAGE / 16;
  static constexpr int SWZ = SLOTS - 1;
  // LDS image of a stage: slot s of stage row R sits at position s ^ swz(R) of
  // the row.  ds_read_b128 serves four groups of 16 lanes, each holding every
  // column row li = 0..15 once, li in {0-3, 12-15} at one lane group lq and li
  // in {4-11} at lq ^ 1; its 64 banks are 16 slots (256 B).
  //  16 slots per row (KS 128): one row per 256 B; slot ^ li is a permutation.
  //   8 slots (KS 64): two rows per 256 B; slot ^ (li & 7) -- li and li ^ 8
  //     share li & 7 but read lq and lq ^ 1 (two positions); li and li ^ 9 read
  //     one position, on rows of different parity (the two halves of the 256 B).
  //   4 slots (KS 32): four rows per 256 B, the rows li, li ^ 4, li ^ 8, li ^ 12
  //     share the quarter: slot ^ g(li >> 2), g = 0, 3, 2, 1, gives them lq, lq
  //     ^ 1 ^ 3, lq ^ 1 ^ 2, lq ^ 1 -- four different slots.
  static constexpr int swz(int row) {
    return SLOTS >= 8 ? row & SWZ : ((row >> 2) & 3) ^ (((row >> 2) & 1) << 1);
  }
  static_assert(SLOTS == 4 || SLOTS == 8 || SLOTS == 16, "swizzles for 4, 8 and 16 slots per row");
  static constexpr int PIECES = STAGE / (W * 1024);  // 1-KiB DMA pieces per wave per stage
  static constexpr int RT = RPW / 16;               // 16-row tiles per wave
  static constexpr int LG = 4;
  // k-steps of v_mfma_f32_16x16x32_f16 (int8: v_mfma_i32_16x16x64_i8, fp4: the
  // scaled 16x16x128) per column tile
  static constexpr int NKS = KW / (FP4 ? 128 : I8 ? 64 : 32);
  static constexpr int NCT = SC / 16;               // column tiles per stage
  // Row-sum chains per row tile.  KS 128: one chain per 64-feature half of the
  // slice (k-steps 2h, 2h + 1 of every column tile, tiles in column order),
  // each folded on its own -- the 4-wave form keeps both in registers, the wide
  // form meets them as its two sub-slices: every KS-128 form sums the same
  // products in the same order, so their bits agree.
  static constexpr int NCH = KW == 128 && !I8 ? 2 : 1;  // (int8: one exact int32 chain)
  // products summed by one row-chain element between two folds (the FOLD
  // columns' tiles, KW / NCH products per tile: 512 at KS 32, 1,024 at KS 64
  // and 128)
  static constexpr int CHAIN = FOLD / 16 * (KW / NCH);
  // ... and the length dal_density_error_bound_sym_d charges the row side with:
  // that of the two-product body (H.H and H.L) these kernels had before, twice
  // CHAIN at the default folds.  The bound's values are part of the interface
  // (pinned by the tests), so it keeps them and over-charges.
  static constexpr int CHARGED = KS == 32 ? DAL_GRAM_CHAIN_MAX / 2 : DAL_GRAM_CHAIN_MAX;
  static_assert(SPF >= 1 && SPP % SPF == 0 && PIECES >= 1 && NKS >= 1, "bad slice");
  static_assert(W == 4 || (W == 8 && KS >= 64), "several super blocks per block: KS >= 64 only");
  static_assert(!WIDE || (W == 8 && KS == (FP4 ? 256 : 128)), "the wide form: 8 waves at KS 128 (fp4: 256)");
  static_assert(FP4 == (KS == 256), "256-feature slices are the fp4 form's");
  static_assert(INT || (NKS % NCH == 0 && KW / NCH == 64 / (KS == 32 ? 2 : 1)),
                "a chain is 64 features of every tile (KS 32: 32)");
  static_assert(INT || CHAIN <= CHARGED, "row chain longer than the density bound charges");
  static_assert(!INT || (WIDE && ROWB == 128 && NSUB == 1 && NKS == 2 && NCH == 1),
                "the int8 and fp4 forms: the wide form over whole slices");
  // int8: |sum_f a_i a_j| < 1.2 * 2^14 per column on unit rows (Cauchy-Schwarz
  // with |32 a| <= |H| + 16 sqrt(d_pad)), so a chain element's FOLD / 4 columns
  // stay below 2^21 and a row's 256 below 2^23: no int32 overflow.
  static_assert(!I8 || FOLD <= 256, "int32 row chains: at most a pair's 256 columns between folds");
  // fp4: a chain element sums FOLD / 16 column tiles x KW features of |a4 a4| <=
  // 144, exact in fp32 whatever the data (gram_fp4.hpp)
  static_assert(!FP4 || (FOLD / 16 * KW * kFp4Max * kFp4Max == kFp4ChainMax &&
                         FOLD * KW * kFp4Max * kFp4Max == kFp4RowMax),
                "fp32 chains of exact integers, int32 row sums");
  // Pairs of one row unit that a chain takes between two folds (round 15).  The
  // integer forms' chains are exact whatever their length, up to the bounds
  // below, and a row unit's rows stay resident for a whole column chunk, so
  // they are folded once per FOLD_PAIRS pairs (and when the rows change:
  // fold_due in gram_schedule.hpp) instead of at the end of every pair, where
  // the fold of waves 0-3 runs with the matrix pipe empty.  The fp32 chains of
  // the fp16 forms round: they keep their fold per pair.  The bounds assume
  // nothing of the operand bytes (gram_fp4.hpp, gram_i8.hpp).
  static constexpr bool CVT_EACH = FP4 && DAL_GRAM_FP4_CVT_EACH != 0;
  static constexpr int FOLD_PAIRS = FP4 ? DAL_GRAM_FOLD_PAIRS_FP4 : I8 ? DAL_GRAM_FOLD_PAIRS_I8 : 1;
  static_assert(FOLD_PAIRS >= 1 && (FOLD_PAIRS == 1 || (WIDE && FOLD == 256)),
                "chains over several pairs: the wide integer forms, one fold group per pair");
  static_assert(!I8 || FOLD_PAIRS <= kI8FoldPairsMax, "int32 row sums over FOLD_PAIRS pairs");
  static_assert(!FP4 || FOLD_PAIRS <= (CVT_EACH ? kFp4FoldPairsMaxEach : kFp4FoldPairsMax),
                "fp32 chains (and a lane's fp32 sum of four) of exact integers over FOLD_PAIRS pairs");

  // the chains' registers and the LDS row accumulator.  fp16: fp32 chains folded
  // to multiples of 2^-32 and added as integers in fp64 (below 2^53: at most
  // 2^21 columns of at most 2^32 each).  int8: the row sum s is an exact int32
  // and adds s * 2^18 (gram_i8.hpp); a column may reach 1.2 * 2^32 here, so the
  // accumulator is an int64 -- exact for any pool the int64 density itself holds.
  using acc4 = typename std::conditional<I8, i32x4, f32x4>::type;
  // (fp4: fp32 chains, converted to int32 at the fold)
  using sum_t = typename std::conditional<INT, int, float>::type;
  using racc_t = typename std::conditional<INT, long long, double>::type;
  // scale: the fp4 form's scale register (kFp4ScaleWord, set once before the pair loop)
  static __device__ __forceinline__ acc4 mfma(f16x8 a, f16x8 b, acc4 c, [[maybe_unused]] int scale) {
    if constexpr (FP4) {
      // (with fp4 on both sides the instruction reads the first four registers of each operand)
      const i32x4 a4 = __builtin_bit_cast(i32x4, a), b4 = __builtin_bit_cast(i32x4, b);
      const i32x8 a8 = {a4[0], a4[1], a4[2], a4[3], 0, 0, 0, 0}, b8 = {b4[0], b4[1], b4[2], b4[3], 0, 0, 0, 0};
      return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, c, 4, 4, 0, scale, 0, scale);
    } else if constexpr (I8) {
      return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b), c, 0,
                                                   0, 0);
    } else {
      return mfma16(a, b, c);
    }
  }
  // A lane's four columns of a row tile.  fp4: every partial sum is an integer
  // of at most 4 x 589,824 = 2,359,296 < 2^24 = 16,777,216, so the fp32 adds are
  // exact (no assumption on the data: kFp4ChainMax) and one v_cvt_i32_f32 per
  // tile takes the sum as it is -- converting each element first would be four.
  // Over FOLD_PAIRS pairs the sum of four stays below 2^24 up to 7 pairs
  // (kFp4FoldPairsMax); CVT_EACH converts the four elements first and adds them
  // as int32, for chains of up to kFp4FoldPairsMaxEach pairs.
  static __device__ __forceinline__ sum_t lane_sum(acc4 m) {
    if constexpr (CVT_EACH)
      return (static_cast<int>(m[0]) + static_cast<int>(m[1])) + (static_cast<int>(m[2]) + static_cast<int>(m[3]));
    else
      return static_cast<sum_t>((m[0] + m[1]) + (m[2] + m[3]));
  }
  static __device__ __forceinline__ void row_add(racc_t* slot, sum_t x) {
    if constexpr (INT)
      atomicAdd(reinterpret_cast<unsigned long long*>(slot),
                static_cast<unsigned long long>(static_cast<long long>(x) << kI8AccShift));
    else
      atomicAdd(slot, static_cast<double>(__builtin_rintf(x * 0x1p8f)));  // units of 2^-24 -> multiples of 2^-32
  }
};
// the wide form's chains are the 4-wave form's (one bound, one set of bits per KS)
static_assert(Cfg<128, 8, 4>::CHAIN == Cfg<128, 4>::CHAIN, "the KS-128 forms define the same chains");

// Unit counters of the chunk-form launches (see the pair loop): next = units
// claimed beyond the G the blocks enter by themselves, done = blocks that
// left.  Library-owned (the interface has no workspace for them), zero at load
// and left zero by every launch's last block.  One slot per launch in flight:
// claim_slot_of hands them out on the host.
struct ClaimSlot {
  unsigned next, done;
};
constexpr int kClaimSlots = 64;
__device__ ClaimSlot g_claim[kClaimSlots];

// Row sums of the taken pairs (the column sums of every pair are added in
// closed form by dal_gram_sym_residual, see the header): for each pair (P,
// J) the taker's rows accumulate <H_i, H_j> over J's 256 columns.
template <int KS, int W, int HVS>
__global__ __launch_bounds__(64 * W, (Cfg<KS, W, HVS>::OCC)) void gram_csym_kernel(
    const uint16_t* __restrict__ urows, int srow0, int n_srb,
    const uint16_t* __restrict__ ucols, int jcol0, int j_lo, int j_hi, int skip_lo, int skip_hi,
    int ns_active, int64_t ldh, int slice_off, int n_slices, int chunk_j, int n_chunks,
    unsigned long long* __restrict__ acc_out, int contig, int claim_slot) {
  using C = Cfg<KS, W, HVS>;
#include "gram_csym_body.inc"
}
// The int8 instance of the wide form (Cfg's I8): the same body, schedule, claim
// and flush protocols; int8 operands, int32 chains, an int64 row accumulator.
__global__ __launch_bounds__(512, 1) void gram_i8sym_kernel(
    const uint16_t* __restrict__ urows, int srow0, int n_srb,
    const uint16_t* __restrict__ ucols, int jcol0, int j_lo, int j_hi, int skip_lo, int skip_hi,
    int ns_active, int64_t ldh, int slice_off, int n_slices, int chunk_j, int n_chunks,
    unsigned long long* __restrict__ acc_out, int contig, int claim_slot) {
  using C = Cfg<128, 8, 4, kFormI8>;
#include "gram_csym_body.inc"
}
// The fp4 instance: the int8 instance's stages and schedule over 256-feature
// slices; e2m1 operands, fp32 chains of exact integers, the same int64 row
// accumulator.
__global__ __launch_bounds__(512, 1) void gram_fp4sym_kernel(
    const uint16_t* __restrict__ urows, int srow0, int n_srb,
    const uint16_t* __restrict__ ucols, int jcol0, int j_lo, int j_hi, int skip_lo, int skip_hi,
    int ns_active, int64_t ldh, int slice_off, int n_slices, int chunk_j, int n_chunks,
    unsigned long long* __restrict__ acc_out, int contig, int claim_slot) {
  using C = Cfg<256, 8, 4, kFormFp4>;
#include "gram_csym_body.inc"
}
// ---------------------------------------------------------------------------
// Residual of the compensation (see the header).  Three launches:
//  1. per super block Q: sigma^H_Q, and the pool total S^L of the L terms,
//     exact int64 in units of 2^-24 (every H and L is a multiple of 2^-24 below
//     2^13);
//  2. per feature: exclusive prefix sums of sigma^H over super blocks of each
//     parity class and their totals, giving S~ and D_B = S^L + CH_B for every
//     requested B (for d_pad <= 64 and few super blocks the launch-3 blocks
//     form them from sigma^H and S^L instead: one launch less, 21 us at
//     configs 2 and 3);
//  3. per row r of the requested super blocks: acc[r] += rint(2^8 *
//     (<L_r, S~> + <H_r, D_B>)) with the dots in fp64 in a fixed order.
// Workspace (the sizes are part of the interface): sig = sigma^H [super
// block][d_pad] int64; rb = d_pad words, S^L as int64 from launch 1, replaced
// by S~ as fp64 by the scan (each feature by the one block that read it,
// behind its barrier); cb = D_B [requested super block][d_pad] fp64.

// One block per (group of super blocks, group of 256 16-byte chunk columns,
// row slice): a super block's 512 operand rows are 512 x CPR 16-byte chunks
// (CPR = ldh / 8 per row: the H and L halves of every slice); thread t reads chunk
// column t % CPR (8 H or 8 L halves of one slice) of rows t / CPR, + 256 /
// CPR, ... -- independent 16-B loads, 8 in flight -- summed exactly in int64,
// then reduced over the threads of the same column in LDS.
// A block walks qg consecutive super blocks: sigma^H of each goes out per
// super block (addresses of its own); the L chunk columns stay in registers
// over the whole walk and reach S^L with one add per block and feature -- S^L
// is d_pad addresses for the whole pool, and one add per super block and row
// slice (15,628 per address at config 4) made this kernel 2.85 ms, from 0.55.
// kForm != fp16: the int8 form's terms (h', l') of gram_i8.hpp, or the fp4
// form's of gram_fp4.hpp, in place of (h, l) -- an L chunk column also reads
// its H chunk (ks halves before it) for h - h'.
template <int kForm>
__device__ __forceinline__ void requant(double& h, double& l) {
  if constexpr (kForm == kFormFp4)
    requant_fp4(h, l);
  else
    requant_i8(h, l);
}
template <int kForm>
__global__ __launch_bounds__(256) void csym_sigma_kernel(const uint16_t* __restrict__ ops, int64_t ldh, int ks,
                                                         int d_pad, int ns, int qg, long long* __restrict__ sig_u,
                                                         long long* __restrict__ sl) {
  __shared__ long long red[256][9];  // [thread][8 halves] (+1: bank spread)
  const int cpr = static_cast<int>(ldh / 8);      // chunks per row
  const int cols = cpr < 256 ? cpr : 256;          // chunk columns of this block
  const int col = blockIdx.y * 256 + threadIdx.x % cols;
  const int rstep = 256 / cols;                    // rows advanced per round
  const int r0 = threadIdx.x / cols;
  // this block's rows of each super block: [rb, re) (gridDim.z row slices)
  const int rb = kSB * static_cast<int>(blockIdx.z) / static_cast<int>(gridDim.z);
  const int re = kSB * (static_cast<int>(blockIdx.z) + 1) / static_cast<int>(gridDim.z);
  // chunk column -> (slice, half, first feature): the row is [slice][H KS | L KS]
  const int hpc = ks / 8;                          // chunks per half of a slice
  const int slice = col / (2 * hpc), within = col % (2 * hpc);
  const int f0 = slice * ks + (within % hpc) * 8;
  const bool l_col = within >= hpc;
  const bool finisher = threadIdx.x < cols && col < cpr;  // thread t < cols finishes chunk column t
  const int q_end = (static_cast<int>(blockIdx.x) + 1) * qg < ns ? (static_cast<int>(blockIdx.x) + 1) * qg : ns;
  long long lsum[8] = {};  // an L column's sums over the block's super blocks
  for (int Q = static_cast<int>(blockIdx.x) * qg; Q < q_end; ++Q) {
    // Summed in fp64, exactly: every term is a multiple of 2^-24 below 2^13 and
    // a thread adds at most kSB of them (< 2^22), so every partial sum has at
    // most 46 significant bits; converted to int64 units once at the end.
    double acc[8] = {};
    if (col < cpr && r0 < rstep) {
      const uint4* base = reinterpret_cast<const uint4*>(ops + static_cast<int64_t>(Q) * kSB * ldh) + col;
      for (int r = rb + r0; r < re; r += 8 * rstep) {
        uint4 q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          q[j] = r + j * rstep < re ? base[static_cast<int64_t>(r + j * rstep) * cpr] : uint4{};
        [[maybe_unused]] uint4 qh[8];  // int8 and fp4 forms, L column: the H chunk of the same features
        if constexpr (kForm != kFormF16) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            qh[j] = l_col && r + j * rstep < re ? base[static_cast<int64_t>(r + j * rstep) * cpr - hpc] : uint4{};
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
          if constexpr (kForm != kFormF16) {
            const uint32_t wh[4] = {qh[j].x, qh[j].y, qh[j].z, qh[j].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const auto term = [e](const uint32_t* v) {
                const uint16_t b = static_cast<uint16_t>(e & 1 ? v[e >> 1] >> 16 : v[e >> 1] & 0xFFFFu);
                return static_cast<double>(static_cast<float>(__builtin_bit_cast(_Float16, b)));
              };
              double h = l_col ? term(wh) : term(w), l = l_col ? term(w) : 0.0;
              requant<kForm>(h, l);
              acc[e] += l_col ? l : h;
            }
            continue;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[2 * e] += static_cast<double>(
                static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(w[e] & 0xFFFFu))));
            acc[2 * e + 1] += static_cast<double>(
                static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(w[e] >> 16))));
          }
        }
      }
    }
    if (l_col) {  // (below 2^35 per super block: int64 holds any pool)
#pragma unroll
      for (int e = 0; e < 8; ++e) lsum[e] += static_cast<long long>(acc[e] * 16777216.0);
    }
    if (Q > static_cast<int>(blockIdx.x) * qg) __syncthreads();  // the previous super block's sums are read
#pragma unroll
    for (int e = 0; e < 8; ++e) red[threadIdx.x][e] = static_cast<long long>(acc[e] * 16777216.0);
    __syncthreads();
    if (finisher && !l_col) {  // sigma^H_Q: sum over the rstep row phases (gridDim.z row slices per address)
      long long v[8] = {};
      for (int p = 0; p < rstep; ++p)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += red[p * cols + threadIdx.x][e];
      long long* dst = sig_u + static_cast<int64_t>(Q) * d_pad + f0;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (v[e] != 0) atomicAdd(reinterpret_cast<unsigned long long*>(dst + e), static_cast<unsigned long long>(v[e]));
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 8; ++e) red[threadIdx.x][e] = lsum[e];
  __syncthreads();
  if (finisher && l_col) {
    long long v[8] = {};
    for (int p = 0; p < rstep; ++p)
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += red[p * cols + threadIdx.x][e];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (v[e] != 0) atomicAdd(reinterpret_cast<unsigned long long*>(sl + f0 + e), static_cast<unsigned long long>(v[e]));
  }
}

// block = kScanWaves waves; lane = one of 64 features (blockIdx.x * 64 +
// lane), wave w owns super blocks [w*ns/kW, (w+1)*ns/kW).  sl: S^L (int64) in
// the d_pad words that st receives S~ in (fp64) -- the same memory; every wave
// reads its feature's S^L before the barrier, wave 0 writes S~ behind it.
// D_B = S^L + CH_B written as fp64 for B in [b0, b1).
#ifndef DAL_CSYM_SCAN_WAVES
#define DAL_CSYM_SCAN_WAVES 16
#endif
constexpr int kScanWaves = DAL_CSYM_SCAN_WAVES;  // super-block ranges per feature (one wave each)
constexpr int kScanBatch = 16;                   // sigma^H loads in flight per thread
#ifndef DAL_CSYM_FUSED_MAX
#define DAL_CSYM_FUSED_MAX 65536  // super blocks x d_pad up to which the residual blocks skip the scan
#endif
__global__ __launch_bounds__(64 * kScanWaves) void csym_scan_kernel(const long long* __restrict__ sig_u, int ns,
                                                                    int d_pad, int b0, int b1, const long long* sl,
                                                                    double* st, double* __restrict__ cb) {
  constexpr int kW = kScanWaves;
  __shared__ long long part[kW][2][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int f = blockIdx.x * 64 + lane;
  const bool live = f < d_pad;
  const int q0 = static_cast<int>(static_cast<int64_t>(ns) * w / kW);
  const int q1 = static_cast<int>(static_cast<int64_t>(ns) * (w + 1) / kW);
  // sigma^H sums per parity class of the super block (even, odd); named
  // registers, not arrays indexed by q & 1 (those would live in scratch)
  // loads in batches of kScanBatch, all in flight before the adds (a wave walks
  // ns / kW super blocks: 244 at config 4)
  long long ue = 0, uo = 0;
  const long long s_l = live ? sl[f] : 0;
  if (live) {
    for (int qb = q0; qb < q1; qb += kScanBatch) {
      long long v[kScanBatch];
#pragma unroll
      for (int j = 0; j < kScanBatch; ++j)
        v[j] = qb + j < q1 ? sig_u[static_cast<int64_t>(qb + j) * d_pad + f] : 0;
#pragma unroll
      for (int j = 0; j < kScanBatch; ++j) {
        const bool odd = (qb + j) & 1;
        ue += odd ? 0 : v[j];
        uo += odd ? v[j] : 0;
      }
    }
  }
  part[w][0][lane] = ue;
  part[w][1][lane] = uo;
  __syncthreads();
  // exclusive prefix over the earlier waves' ranges, and the totals
  long long eue = 0, euo = 0, tue = 0, tuo = 0;
  for (int v = 0; v < kW; ++v) {
    const long long a0 = part[v][0][lane], a1 = part[v][1][lane];
    if (v < w) {
      eue += a0;
      euo += a1;
    }
    tue += a0;
    tuo += a1;
  }
  if (!live) return;
  // S~ = the sum of H + L over every row
  if (w == 0) st[f] = static_cast<double>(tue + tuo + s_l);
  for (int qb = q0; qb < q1; qb += kScanBatch) {
    long long v[kScanBatch];
#pragma unroll
    for (int j = 0; j < kScanBatch; ++j)
      v[j] = qb + j < q1 ? sig_u[static_cast<int64_t>(qb + j) * d_pad + f] : 0;
#pragma unroll
    for (int j = 0; j < kScanBatch; ++j) {
      const int q = qb + j;
      // e* = exclusive prefix (super blocks < q) per class; b = q's class
      const bool odd = q & 1;
      if (q < q1 && q >= b0 && q < b1) {
        // CH_B = sum_{P < B, same class} + sum_{P > B, other class} of sigma^H
        // (the other super blocks that take B: B takes itself, the later ones
        // of its class and the earlier ones of the other, whose H.H row sums
        // the MFMAs formed)
        const long long ch = odd ? (euo + tue - eue) : (eue + tuo - euo);
        cb[static_cast<int64_t>(q - b0) * d_pad + f] = static_cast<double>(ch + s_l);
      }
      eue += odd ? 0 : v[j];
      euo += odd ? v[j] : 0;
    }
  }
}

// One thread per row: a block's 256 rows lie in one super block B; S~ and B's
// D_B = S^L + CH_B are staged in LDS once; each thread sums its row's features
// in order, t = t + l_f S~_f, t = t + h_f D_f for f = 0, 1, ... (fp64, no FMA;
// sums of products only, S~ and D_B being formed as integers) -- a fixed
// order, so the bits are the same on every GPU count.  rows:
// the operand of the requested super blocks.  The rows reach the threads
// through LDS, kResFeat features at a time: the block reads each row's H and L
// runs of those features with coalesced 16-B loads (consecutive threads,
// consecutive chunks of one row), so every fetched line is used at once.
// (Round 5 before: each thread read its own row 16 B at a time, 64 rows one
// ldh apart per wave instruction -- the lines left L2 before their other
// chunks were read, 2.2 ms for config 4's 2 GB operand.  Round 4: one wave per
// row, lanes over features and a butterfly -- 2-byte loads.)
constexpr int kResRows = 256;
constexpr int kResFeat = 32;                 // features per LDS stage (divides every KS)
constexpr int kResQ = kResFeat / 4;          // 16-B chunks per row per stage: H kResFeat/8, L kResFeat/8
constexpr int kResLd = kResQ + 1;            // LDS row stride in 16-B chunks (+1: the threads' rows spread over the banks)
// kMode kResFused (d_pad 32 or 64, few super blocks): no scan launch -- every
// block forms its own S~ and D_B from sigma^H and S^L (256 / d_pad thread
// groups over the super blocks, exact int64 sums reduced in LDS; the same
// integers as the scan's; st then still holds S^L as int64).  kResStaged: the
// scan's S~, D_B staged in LDS (16 d_pad bytes).
// kResGlobal (d_pad > kResLdsMaxFeat, where they would not fit beside the
// tile): read in place from the scan's output, uniform addresses.
constexpr int kResStaged = 0, kResFused = 1, kResGlobal = 2;
constexpr int kResLdsMaxFeat = 1024;  // 16 KiB of S~ | D_B + the 36 KiB tile: within 64 KiB per block
// kForm != fp16: (h, l) -> the int8 or fp4 form's (h', l') (gram_i8.hpp, gram_fp4.hpp), nothing else.
template <int kMode, int kForm = kFormF16>
__global__ __launch_bounds__(kResRows) void csym_residual_kernel(const uint16_t* __restrict__ rows, int64_t ldh, int ks,
                                                                 int d_pad, int b0, int n_rows,
                                                                 const double* __restrict__ st,
                                                                 const double* __restrict__ cb,
                                                                 const long long* __restrict__ sig_u, int ns,
                                                                 long long* __restrict__ acc) {
  extern __shared__ double rc[];  // [d_pad] S~ | [d_pad] D_B
  __shared__ uint4 tile[kResRows * kResLd];
  const int tid = threadIdx.x;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * kResRows;  // (a multiple of 256: one super block)
  const int64_t B = r0 / kSB;                                       // relative to b0
  if constexpr (kMode == kResFused) {
    // feature pairs (16-B loads of sigma^H): 256 / (d_pad / 2) thread groups
    // over the super blocks -- 8 (d_pad 64) or 16 (d_pad 32)
    __shared__ long long red[8][kResRows];
    const int qB = b0 + static_cast<int>(B);  // this block's super block
    const int hp = d_pad / 2, G = kResRows / hp, fp = tid % hp, grp = tid / hp;
    long long pe[2] = {}, po[2] = {}, te[2] = {}, to[2] = {};  // per class: sums over super blocks < qB, and totals
    const longlong2* su2 = reinterpret_cast<const longlong2*>(sig_u);
    for (int qb = grp; qb < ns; qb += kScanBatch * G) {
      longlong2 v[kScanBatch];
#pragma unroll
      for (int j = 0; j < kScanBatch; ++j) {
        const int q = qb + j * G;
        v[j] = q < ns ? su2[static_cast<int64_t>(q) * hp + fp] : longlong2{0, 0};
      }
#pragma unroll
      for (int j = 0; j < kScanBatch; ++j) {
        const int q = qb + j * G;
        const bool odd = q & 1, before = q < qB;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const long long x = c ? v[j].y : v[j].x;
          te[c] += odd ? 0 : x;
          to[c] += odd ? x : 0;
          pe[c] += before && !odd ? x : 0;
          po[c] += before && odd ? x : 0;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      red[4 * c][tid] = pe[c];
      red[4 * c + 1][tid] = po[c];
      red[4 * c + 2][tid] = te[c];
      red[4 * c + 3][tid] = to[c];
    }
    __syncthreads();
    if (tid < hp) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        long long eue = 0, euo = 0, tue = 0, tuo = 0;
        for (int g = 0; g < G; ++g) {
          eue += red[4 * c][g * hp + tid];
          euo += red[4 * c + 1][g * hp + tid];
          tue += red[4 * c + 2][g * hp + tid];
          tuo += red[4 * c + 3][g * hp + tid];
        }
        const bool odd = qB & 1;  // S~, CH_B as in csym_scan_kernel
        const int f = 2 * tid + c;
        const long long s_l = reinterpret_cast<const long long*>(st)[f];
        rc[f] = static_cast<double>(tue + tuo + s_l);
        rc[d_pad + f] = static_cast<double>((odd ? (euo + tue - eue) : (eue + tuo - euo)) + s_l);
      }
    }
  } else if constexpr (kMode == kResStaged) {
    for (int f = tid; f < d_pad; f += kResRows) {
      rc[f] = st[f];
      rc[d_pad + f] = cb[B * d_pad + f];
    }
  }
  const double* __restrict__ Sv = kMode == kResGlobal ? st : rc;
  const double* __restrict__ Dv = kMode == kResGlobal ? cb + B * d_pad : rc + d_pad;
  const int live_rows = n_rows - r0 < kResRows ? static_cast<int>(n_rows - r0) : kResRows;
  const uint16_t* blk = rows + r0 * ldh;
  double t = 0.0;
  for (int f0 = 0; f0 < d_pad; f0 += kResFeat) {
    // the stage's H run starts at halves (f0 / ks) * 2 ks + f0 % ks, its L run ks later
    const int64_t hoff = static_cast<int64_t>(f0 / ks) * 2 * ks + f0 % ks;
    uint4 q[kResQ];
#pragma unroll
    for (int j = 0; j < kResQ; ++j) {
      const int e = tid + kResRows * j;
      const int r = e / kResQ, c = e % kResQ;  // row of the block, chunk of the stage (H first, then L)
      const int64_t off = r * ldh + hoff + (c < kResQ / 2 ? c * 8 : ks + (c - kResQ / 2) * 8);
      q[j] = r < live_rows ? *reinterpret_cast<const uint4*>(blk + off) : uint4{};
    }
    if (f0) __syncthreads();  // the previous stage's tile is consumed
#pragma unroll
    for (int j = 0; j < kResQ; ++j) {
      const int e = tid + kResRows * j;
      tile[(e / kResQ) * kResLd + e % kResQ] = q[j];
    }
    __syncthreads();
    if (tid < live_rows) {
#pragma unroll
      for (int c = 0; c < kResQ / 2; ++c) {
        const uint4 hq = tile[tid * kResLd + c], lq = tile[tid * kResLd + kResQ / 2 + c];
        const uint32_t hw[4] = {hq.x, hq.y, hq.z, hq.w}, lw[4] = {lq.x, lq.y, lq.z, lq.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int f = f0 + c * 8 + e;
          const uint16_t hb = static_cast<uint16_t>(e & 1 ? hw[e >> 1] >> 16 : hw[e >> 1] & 0xFFFFu);
          const uint16_t lb = static_cast<uint16_t>(e & 1 ? lw[e >> 1] >> 16 : lw[e >> 1] & 0xFFFFu);
          const double h = static_cast<double>(static_cast<float>(__builtin_bit_cast(_Float16, hb)));
          const double l = static_cast<double>(static_cast<float>(__builtin_bit_cast(_Float16, lb)));
          if constexpr (kForm != kFormF16) {
            double h8 = h, l8 = l;
            requant<kForm>(h8, l8);
            t = t + l8 * Sv[f];
            t = t + h8 * Dv[f];
            continue;
          }
          t = t + l * Sv[f];
          t = t + h * Dv[f];
        }
      }
    }
  }
  // S~, D_B in units of 2^-24 x (split units); value = t * 2^-24 * 2^-24 ... in
  // fixed point (2^32): t * 2^-24 (operand units^2 = 2^24 x value) * 2^8
  if (tid < live_rows && t != 0.0)
    acc[static_cast<int64_t>(b0) * kSB + r0 + tid] += static_cast<long long>(__builtin_rint(t * 0x1p-16));
}

// ---------------------------------------------------------------------------
// a(H) of the split operand (gram_i8.hpp): thread t takes 16 features of a row
// -- 32 B of its slice's H run in, 16 B out, rows [n_rows][d_pad] int8 in
// feature order.
__global__ __launch_bounds__(256) void quant_i8_kernel(const uint16_t* __restrict__ ops, int64_t n_chunks, int d_pad,
                                                       int ks, int8_t* __restrict__ out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= n_chunks) return;
  const int cpr = d_pad / 16;
  const int64_t row = t / cpr;
  const int f0 = static_cast<int>(t % cpr) * 16;
  const uint4* src = reinterpret_cast<const uint4*>(ops + row * 2 * d_pad + (f0 / ks) * 2 * ks + f0 % ks);
  const uint4 q[2] = {src[0], src[1]};
  uint32_t o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint4 v = q[k >> 1];
    const uint32_t w[2] = {k & 1 ? v.z : v.x, k & 1 ? v.w : v.y};
    uint32_t b = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint16_t hb = static_cast<uint16_t>(e & 1 ? w[e >> 1] >> 16 : w[e >> 1] & 0xFFFFu);
      b |= static_cast<uint32_t>(quant_i8(static_cast<float>(__builtin_bit_cast(_Float16, hb))) & 0xFF) << (8 * e);
    }
    o[k] = b;
  }
  reinterpret_cast<uint4*>(out)[t] = uint4{o[0], o[1], o[2], o[3]};
}

// The e2m1 codes of a4(H) (gram_fp4.hpp): thread t takes 32 features of a row
// -- 64 B of its 128-slice's H run in, 16 B out, rows [n_rows][d_pad / 2] bytes
// in feature order, the even feature in the low nibble.
__global__ __launch_bounds__(256) void quant_fp4_kernel(const uint16_t* __restrict__ ops, int64_t n_chunks, int d_pad,
                                                        int ks, uint8_t* __restrict__ out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= n_chunks) return;
  const int cpr = d_pad / 32;
  const int64_t row = t / cpr;
  const int f0 = static_cast<int>(t % cpr) * 32;
  const uint4* src = reinterpret_cast<const uint4*>(ops + row * 2 * d_pad + (f0 / ks) * 2 * ks + f0 % ks);
  const uint4 q[4] = {src[0], src[1], src[2], src[3]};
  uint32_t o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // 8 features -> one word
    const uint32_t w[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
    uint32_t b = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint16_t hb = static_cast<uint16_t>(e & 1 ? w[e >> 1] >> 16 : w[e >> 1] & 0xFFFFu);
      b |= code_fp4(quant_fp4(static_cast<float>(__builtin_bit_cast(_Float16, hb)))) << (4 * e);
    }
    o[k] = b;
  }
  reinterpret_cast<uint4*>(out)[t] = uint4{o[0], o[1], o[2], o[3]};
}

// ---------------------------------------------------------------------------
int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 256;
  return cus;
}

// The fewest column chunks choose_chunks (gram_schedule.hpp) may pick for the
// round-robin units.  KS 64 with a column operand of <= DAL_GRAM_SMALL_MB
// (in L2 + MALL whole) takes >= 2 chunks instead of the contiguous schedule:
// 100k x 64 (25.6 MB) 1.6-4.7 % faster in two of three same-process runs
// (+0.7 % in the third), the clock 1.83 -> 1.88-1.92 GHz; at KS 32 and 128 the
// same change lost (60k x 32 +7.4 %, 20k x 256 +4.3 %; round 6,
// profiles/r06/pmc/clock_ab_chunk_counts.txt).
#ifndef DAL_GRAM_MIN_CHUNKS
#define DAL_GRAM_MIN_CHUNKS 16
#endif
#ifndef DAL_GRAM_SMALL_MB
#define DAL_GRAM_SMALL_MB 32
#endif
#ifndef DAL_GRAM_MIN_CHUNKS_SMALL
#define DAL_GRAM_MIN_CHUNKS_SMALL 2
#endif
// The wide form (8 waves, one block per CU, four super blocks per block: each
// B stage feeds 2,048 rows, a quarter of the L2 -> LDS bytes per flop of the
// 4-wave form) for the round-robin schedule at KS 128; 0: the 4-wave form.
#ifndef DAL_GRAM_WAVES8
#define DAL_GRAM_WAVES8 1
#endif

// The counter slot of a chunk-form launch on `stream`, -1: none (the launch
// then deals its units statically; the bits are the same).  Two launches may
// share a slot only if they cannot be in flight together, and launches on one
// stream run in order, so every stream keeps a slot of its own for the life
// of the process: at most kClaimSlots streams get one, whatever the host
// threads that launch on them.  g_claim exists once per device and a stream
// belongs to one device, so devices need no slots of their own.
// hipStreamPerThread is one handle for a stream per host thread and gets
// none.  (A graph replays with the slot of the stream it was captured on: do
// not replay it beside launches on that stream.)
int claim_slot_of(hipStream_t stream) {
  static std::mutex mu;
  static hipStream_t owner[kClaimSlots];
  static int n_owners = 0;
  if (stream == hipStreamPerThread) return -1;
  std::lock_guard<std::mutex> lock(mu);
  for (int i = 0; i < n_owners; ++i)
    if (owner[i] == stream) return i;
  if (n_owners == kClaimSlots) return -1;
  owner[n_owners] = stream;
  return n_owners++;
}

// n_slices feature slices from slice_off on in one launch (chunk form; the
// contiguous form takes one slice per launch).
template <int KS, int W, int HVS = W / 4>
int launch_csym_w(const uint16_t* rows, int64_t srow0, int64_t n_srb, const uint16_t* cols, int64_t jcol0,
                  int64_t j_lo, int64_t j_hi, int64_t skip_lo, int64_t skip_hi, int64_t ns_active, int64_t ldh,
                  int slice_off, int n_slices, int64_t* acc, int grid_blocks, int contig, int64_t min_chunks,
                  hipStream_t stream) {
  // grid_blocks counts 4-wave blocks (two per CU); 8-wave blocks are one per CU
  using C = Cfg<KS, W, HVS>;
  constexpr int kOcc = C::OCC;
  const int G0r = W == 4 ? (grid_blocks > 0 ? grid_blocks * kOcc / 2 : kOcc * device_cus())
                         : (grid_blocks > 0 ? grid_blocks : 2 * device_cus()) * 4 / W * kOcc;
  const int G0 = G0r > 0 ? G0r : 1;  // (a one-block grid in the 8-wave form)
  if (!GramSchedule<HVS>::form_ok(contig)) return DAL_ERR_ARG;
  const GramLaunch L = plan_launch<HVS>(srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi, ns_active, G0, contig, min_chunks,
                                        n_slices * C::NSUB);
  if (L.G <= 0) return DAL_OK;
  if (contig && n_slices != 1) return DAL_ERR_ARG;
  // units beyond the G the blocks enter by themselves are claimed from a counter (none left: no counter)
  const int slot = !contig && L.units > L.G ? claim_slot_of(stream) : -1;
  hipLaunchKernelGGL((gram_csym_kernel<KS, W, HVS>), dim3(static_cast<unsigned>(L.G)), dim3(64 * W), 0, stream, rows,
                     static_cast<int>(srow0), static_cast<int>(n_srb), cols, static_cast<int>(jcol0),
                     static_cast<int>(j_lo), static_cast<int>(j_hi), static_cast<int>(skip_lo),
                     static_cast<int>(skip_hi), static_cast<int>(ns_active), ldh, slice_off, n_slices, L.chunk_j,
                     L.n_chunks, reinterpret_cast<unsigned long long*>(acc), contig, slot);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

// The int8 and fp4 forms: every slice in one round-robin launch of
// gram_i8sym_kernel or gram_fp4sym_kernel (units count whole slices), also for
// a small column range.  ld2: the operand's row stride in 2-byte units (int8:
// d_pad / 2, fp4: d_pad / 4).
template <int FORM>
int launch_intsym(const void* rows, int64_t srow0, int64_t n_srb, const void* cols, int64_t jcol0, int64_t j_lo,
                  int64_t j_hi, int64_t skip_lo, int64_t skip_hi, int64_t ns_active, int64_t ld2, int n_slices,
                  int64_t* acc, int grid_blocks, int64_t min_chunks, hipStream_t stream) {
  using C = Cfg<FORM == kFormFp4 ? 256 : 128, 8, 4, FORM>;
  const int G0r = (grid_blocks > 0 ? grid_blocks : 2 * device_cus()) / 2;  // grid_blocks counts 4-wave blocks
  const int G0 = G0r > 0 ? G0r : 1;
  const GramLaunch L = plan_launch<C::HALVES>(srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi, ns_active, G0, 0, min_chunks,
                                              n_slices * C::NSUB);
  if (L.G <= 0) return DAL_OK;
  const int slot = L.units > L.G ? claim_slot_of(stream) : -1;
  hipLaunchKernelGGL(FORM == kFormFp4 ? gram_fp4sym_kernel : gram_i8sym_kernel, dim3(static_cast<unsigned>(L.G)),
                     dim3(C::NT), 0, stream,
                     reinterpret_cast<const uint16_t*>(rows), static_cast<int>(srow0), static_cast<int>(n_srb),
                     reinterpret_cast<const uint16_t*>(cols), static_cast<int>(jcol0), static_cast<int>(j_lo),
                     static_cast<int>(j_hi), static_cast<int>(skip_lo), static_cast<int>(skip_hi),
                     static_cast<int>(ns_active), ld2, 0, n_slices, L.chunk_j, L.n_chunks,
                     reinterpret_cast<unsigned long long*>(acc), 0, slot);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

#ifndef DAL_GRAM_CONTIG_MB
#define DAL_GRAM_CONTIG_MB 32  // column operands up to this size take the contiguous schedule (KS 32, 128)
#endif
#ifndef DAL_GRAM_KS64_CHUNKED
#define DAL_GRAM_KS64_CHUNKED 1  // ... KS 64 takes >= DAL_GRAM_MIN_CHUNKS_SMALL column chunks instead
#endif
template <int KS>
int launch_csym(const uint16_t* rows, int64_t srow0, int64_t n_srb, const uint16_t* cols, int64_t jcol0,
                int64_t j_lo, int64_t j_hi, int64_t skip_lo, int64_t skip_hi, int64_t ns_active, int64_t ldh,
                int n_slices, int64_t* acc, int grid_blocks, hipStream_t stream) {
  // contiguous equal shares of the pair grid per block for a small column
  // operand (<= 32 MB at KS 32 / 128), else round-robin column chunks whose
  // blocks sweep the same column stages together (a small KS-64 operand in as
  // few as two chunks).  Exact integer accumulation: the schedule never
  // changes the bits.
  const int64_t col_bytes = (j_hi - j_lo) * 256 * ldh * 2;
  const bool small = col_bytes <= (int64_t{DAL_GRAM_SMALL_MB} << 20);
  const int contig = col_bytes <= (int64_t{DAL_GRAM_CONTIG_MB} << 20) && !(KS == 64 && DAL_GRAM_KS64_CHUNKED);
  const int64_t min_chunks = small ? DAL_GRAM_MIN_CHUNKS_SMALL : DAL_GRAM_MIN_CHUNKS;
  // the chunk form covers every slice in one launch, the contiguous form one slice per launch
  const int per_launch = contig ? 1 : n_slices;
  for (int s0 = 0; s0 < n_slices; s0 += per_launch) {
    const int so = s0 * 2 * KS;  // halves: slice s starts at s * 2 * KS
    int rc;
    if constexpr ((KS == 128 && DAL_GRAM_WAVES8) || (KS == 64 && DAL_GRAM_W8_KS64))
      if (!contig) {
        // KS 128: the wide form (four super blocks per block over 64-feature sub-slices)
        rc = launch_csym_w<KS, 8, KS == 128 ? 4 : 2>(rows, srow0, n_srb, cols, jcol0, j_lo, j_hi, skip_lo, skip_hi,
                                                     ns_active, ldh, so, per_launch, acc, grid_blocks, contig,
                                                     min_chunks, stream);
        if (rc != DAL_OK) return rc;
        continue;
      }
    rc = launch_csym_w<KS, 4>(rows, srow0, n_srb, cols, jcol0, j_lo, j_hi, skip_lo, skip_hi, ns_active, ldh, so,
                              per_launch, acc, grid_blocks, contig, min_chunks, stream);
    if (rc != DAL_OK) return rc;
  }
  return DAL_OK;
}

struct ResidualLayout {
  size_t sig_u, rb, cb, total;
};
ResidualLayout residual_layout(int64_t ns_active, int64_t n_srb, int64_t d_pad) {
  ResidualLayout L{};
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += (bytes + 255) / 256 * 256;
    return at;
  };
  L.sig_u = take(static_cast<size_t>(ns_active * d_pad) * 8);
  L.rb = take(static_cast<size_t>(n_srb * d_pad) * 8);
  L.cb = take(static_cast<size_t>(n_srb * d_pad) * 8);
  L.total = o;
  return L;
}

}  // namespace

int split_ks(int64_t d_pad) { return d_pad == 32 ? 32 : (d_pad % 128 == 0 ? 128 : 64); }

}  // namespace dal

using namespace dal;

namespace {
// Row-side chain length the bound charges the kernel that runs d_pad
// (split_ks) with, 0 = the longest over every KS (Cfg::CHARGED: twice the
// kernel's own Cfg::CHAIN at the default folds, never below it).
int row_chain_products(int64_t d_pad) {
  if (d_pad <= 0) {
    int m = Cfg<32, 4>::CHARGED;
    m = Cfg<64, 4>::CHARGED > m ? Cfg<64, 4>::CHARGED : m;
    return Cfg<128, 4>::CHARGED > m ? Cfg<128, 4>::CHARGED : m;
  }
  const int ks = split_ks(d_pad);
  return ks == 32 ? Cfg<32, 4>::CHARGED : ks == 64 ? Cfg<64, 4>::CHARGED : Cfg<128, 4>::CHARGED;
}
}  // namespace

extern "C" double dal_density_error_bound_sym_d(int64_t n_cols, int64_t d_pad) {
  // dal_gram_rowsum_sym + dal_gram_sym_residual against the canonical fp64
  // density, per density entry (one column j of row i), u = 2^-23 (a
  // conservative unit roundoff for the MFMA's internal fp32 adds, counted as
  // sequential adds), products exact (f16 x f16), c = 1 + 2^-8 >= sum_d |h_i
  // h_j| over sum_d |u_i u_j| <= 1 (Cauchy-Schwarz on unit rows):
  //   row side   (the MFMA row sums of the taken pairs) NCH chains per row
  //              tile between folds, charged Cfg<KS>::CHARGED products each
  //              (1,024 at KS 32, 2,048 at KS 64 and 128: the chains of the
  //              earlier H.H + H.L body; the H.H chains are Cfg<KS>::CHAIN =
  //              FOLD / 16 / NCH tiles x KS, half as long, so this over-charges
  //              -- the bound's values are part of the interface and stay), 3
  //              adds in the lane and 2 across lanes over a row's 16 columns:
  //              gamma_(CHARGED + 5) * c
  //   column side  none: every taken pair's column sums and the L terms are
  //              the closed form <L_i, S~> + <H_i, S^L + CH_B> of
  //              dal_gram_sym_residual (exact int64 sums, an fp64 dot): below
  //              2^-40 per column together
  //   split + fp32 unit rows  5 * 2^-22;  fixed-point roundings <= 2^-33 each
  const double u = 1.0 / 8388608.0;  // 2^-23
  auto gamma = [u](double n) { return n * u / (1.0 - n * u); };
  const double s = 1.0 / 4194304.0;  // 2^-22
  const double row = gamma(static_cast<double>(row_chain_products(d_pad)) + 5.0);
  const double c = 1.0 + 1.0 / 256.0;
  return (row * c + 5.0 * s + 1e-10) * static_cast<double>(n_cols) + 1e-9;
}

// Feature-width-free form (ABI v5): the bound of the longest row chain of any
// KS, valid for every pool.
extern "C" double dal_density_error_bound_sym(int64_t n_cols) { return dal_density_error_bound_sym_d(n_cols, 0); }

extern "C" int dal_gram_rowsum_sym_skip(const uint16_t* rows, int64_t row_block0, int64_t n_row_blocks,
                                        const uint16_t* cols, int64_t col_block0, int64_t j_lo, int64_t j_hi,
                                        int64_t skip_lo, int64_t skip_hi, int64_t nb_active, int64_t d_pad,
                                        int64_t* acc, int grid_blocks, dal_stream_t stream) {
  if (!rows || !cols || !acc) return DAL_ERR_ARG;
  if (row_block0 < 0 || n_row_blocks <= 0 || col_block0 < 0 || nb_active <= 0) return DAL_ERR_SHAPE;
  if (j_lo < col_block0 || j_hi < j_lo || j_hi > nb_active || skip_hi < skip_lo) return DAL_ERR_SHAPE;
  if (d_pad != dal_pad_features(d_pad)) return DAL_ERR_SHAPE;
  if ((row_block0 | n_row_blocks | nb_active) & 1) return DAL_ERR_SHAPE;  // whole 512-row super blocks
  if ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(cols)) & 15) return DAL_ERR_SHAPE;
  if (j_hi == j_lo || row_block0 >= nb_active) return DAL_OK;
  hipStream_t st = as_stream(stream);
  const int ks = split_ks(d_pad);
  const int64_t ldh = 2 * d_pad;
  const int n_slices = static_cast<int>(d_pad / ks);
  const int64_t s0 = row_block0 / 2, ns = n_row_blocks / 2, na = nb_active / 2;
  if (ks == 32)
    return launch_csym<32>(rows, s0, ns, cols, col_block0, j_lo, j_hi, skip_lo, skip_hi, na, ldh, n_slices, acc,
                           grid_blocks, st);
  if (ks == 64)
    return launch_csym<64>(rows, s0, ns, cols, col_block0, j_lo, j_hi, skip_lo, skip_hi, na, ldh, n_slices, acc,
                           grid_blocks, st);
  return launch_csym<128>(rows, s0, ns, cols, col_block0, j_lo, j_hi, skip_lo, skip_hi, na, ldh, n_slices, acc,
                          grid_blocks, st);
}

extern "C" int dal_gram_rowsum_sym(const uint16_t* rows, int64_t row_block0, int64_t n_row_blocks,
                                   const uint16_t* cols, int64_t col_block0, int64_t j_lo, int64_t j_hi,
                                   int64_t nb_active, int64_t d_pad, int64_t* acc, int grid_blocks,
                                   dal_stream_t stream) {
  return dal_gram_rowsum_sym_skip(rows, row_block0, n_row_blocks, cols, col_block0, j_lo, j_hi, 0, 0, nb_active,
                                  d_pad, acc, grid_blocks, stream);
}

extern "C" size_t dal_gram_sym_residual_workspace_bytes(int64_t nb_active, int64_t n_row_blocks, int64_t d_pad) {
  if (nb_active <= 0 || n_row_blocks <= 0 || d_pad <= 0) return 0;
  return residual_layout(nb_active / 2, n_row_blocks / 2, d_pad).total;
}

namespace {
// kForm != fp16: the closed form of the int8 or fp4 form's terms (h', l'), gram_i8.hpp / gram_fp4.hpp
template <int kForm>
int gram_sym_residual(const uint16_t* ops, int64_t nb_active, int64_t row_block0, int64_t n_row_blocks, int64_t d_pad,
                      int64_t* acc, void* ws, size_t ws_bytes, dal_stream_t stream,
                      const int64_t* pre_sigma_h = nullptr, const int64_t* pre_s_l = nullptr) {
  if (!ops || !acc || !ws) return DAL_ERR_ARG;
  if (nb_active <= 0 || row_block0 < 0 || n_row_blocks <= 0 || ((row_block0 | n_row_blocks | nb_active) & 1))
    return DAL_ERR_SHAPE;
  if (d_pad != dal_pad_features(d_pad) || (reinterpret_cast<uintptr_t>(ops) & 15) ||
      (reinterpret_cast<uintptr_t>(ws) & 255))
    return DAL_ERR_SHAPE;
  const int64_t na = nb_active / 2, s0 = row_block0 / 2;
  int64_t ns = n_row_blocks / 2;
  if (s0 >= na) return DAL_OK;
  if (s0 + ns > na) ns = na - s0;  // padding super blocks past the pool hold no rows
  const ResidualLayout L = residual_layout(na, n_row_blocks / 2, d_pad);
  if (ws_bytes < L.total) return DAL_ERR_SHAPE;
  hipStream_t st = as_stream(stream);
  unsigned char* w = static_cast<unsigned char*>(ws);
  long long* sig_u = reinterpret_cast<long long*>(w + L.sig_u);
  double* rb = reinterpret_cast<double*>(w + L.rb);
  double* cb = reinterpret_cast<double*>(w + L.cb);
  const int ks = split_ks(d_pad);
  const int64_t ldh = 2 * d_pad;
  // sigma^H and, behind it (the layout's padding between), the d_pad words of S^L
  static_assert(sizeof(long long) == sizeof(double), "S^L and S~ share their words");
  long long* sl = reinterpret_cast<long long*>(rb);
  if (pre_sigma_h) {  // launch 1 already ran (dal_prep_split_fp4): the caller's sums, read in place
    sig_u = const_cast<long long*>(reinterpret_cast<const long long*>(pre_sigma_h));
    sl = const_cast<long long*>(reinterpret_cast<const long long*>(pre_s_l));
  } else {
    if (hipMemsetAsync(sig_u, 0, L.rb - L.sig_u + static_cast<size_t>(d_pad) * 8, st) != hipSuccess)
      return DAL_ERR_HIP;
    // rows of a super block over 4 blocks (more loads in flight: 196 super blocks at config 2);
    // super blocks per block: what leaves about four blocks per CU, at most 32
    const int64_t ny = ceil_div(ldh / 8, 256);
    const int64_t qg0 = na * ny * 4 / (4 * device_cus()), qg = qg0 < 1 ? 1 : qg0 > 32 ? 32 : qg0;
    hipLaunchKernelGGL(csym_sigma_kernel<kForm>,
                       dim3(static_cast<unsigned>(ceil_div(na, qg)), static_cast<unsigned>(ny), 4), dim3(256), 0, st,
                       ops, ldh, ks, static_cast<int>(d_pad), static_cast<int>(na), static_cast<int>(qg), sig_u, sl);
    DAL_RETURN_IF_LAUNCH_FAILED();
  }
  const int64_t n_rows = ns * kSB;
  const dim3 grid(static_cast<unsigned>(ceil_div(n_rows, kResRows)));
  const size_t smem = static_cast<size_t>(2 * d_pad) * 8;
  const uint16_t* rows = ops + s0 * kSB * ldh;
  if (kForm == kFormF16 && d_pad <= 64 && na * d_pad <= DAL_CSYM_FUSED_MAX) {  // the blocks form S~, D_B themselves
    hipLaunchKernelGGL(csym_residual_kernel<kResFused>, grid, dim3(kResRows), smem, st, rows, ldh, ks,
                       static_cast<int>(d_pad), static_cast<int>(s0), static_cast<int>(n_rows), rb, cb, sig_u,
                       static_cast<int>(na), reinterpret_cast<long long*>(acc));
  } else {
    hipLaunchKernelGGL(csym_scan_kernel, dim3(static_cast<unsigned>(ceil_div(d_pad, 64))), dim3(64 * kScanWaves), 0,
                       st, sig_u, static_cast<int>(na), static_cast<int>(d_pad), static_cast<int>(s0),
                       static_cast<int>(s0 + ns), sl, rb, cb);
    DAL_RETURN_IF_LAUNCH_FAILED();
    if (d_pad <= kResLdsMaxFeat) {
      hipLaunchKernelGGL((csym_residual_kernel<kResStaged, kForm>), grid, dim3(kResRows), smem, st, rows, ldh, ks,
                         static_cast<int>(d_pad), static_cast<int>(s0), static_cast<int>(n_rows), rb, cb, sig_u,
                         static_cast<int>(na), reinterpret_cast<long long*>(acc));
    } else {  // wide pools: S~, D_B read in place (they would not fit in LDS beside the tile)
      hipLaunchKernelGGL((csym_residual_kernel<kResGlobal, kForm>), grid, dim3(kResRows), 0, st, rows, ldh, ks,
                         static_cast<int>(d_pad), static_cast<int>(s0), static_cast<int>(n_rows), rb, cb, sig_u,
                         static_cast<int>(na), reinterpret_cast<long long*>(acc));
    }
  }
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}
}  // namespace

extern "C" int dal_gram_sym_residual(const uint16_t* ops, int64_t nb_active, int64_t row_block0, int64_t n_row_blocks,
                                     int64_t d_pad, int64_t* acc, void* ws, size_t ws_bytes, dal_stream_t stream) {
  return gram_sym_residual<kFormF16>(ops, nb_active, row_block0, n_row_blocks, d_pad, acc, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------
// The int8 form (gram_i8.hpp; KS 128 pools).
extern "C" int dal_quant_i8(const uint16_t* ops, int64_t n_rows, int64_t d_pad, int8_t* out_i8, dal_stream_t stream) {
  if (!ops || !out_i8) return DAL_ERR_ARG;
  if (n_rows < 0 || d_pad <= 0 || d_pad % 128 || d_pad != dal_pad_features(d_pad)) return DAL_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(ops) | reinterpret_cast<uintptr_t>(out_i8)) & 15) return DAL_ERR_SHAPE;
  if (n_rows == 0) return DAL_OK;
  const int64_t n_chunks = n_rows * (d_pad / 16);
  hipLaunchKernelGGL(quant_i8_kernel, dim3(static_cast<unsigned>(ceil_div(n_chunks, 256))), dim3(256), 0,
                     as_stream(stream), ops, n_chunks, static_cast<int>(d_pad), split_ks(d_pad), out_i8);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

extern "C" int dal_gram_rowsum_sym_i8_skip(const int8_t* rows_i8, int64_t row_block0, int64_t n_row_blocks,
                                           const int8_t* cols_i8, int64_t col_block0, int64_t j_lo, int64_t j_hi,
                                           int64_t skip_lo, int64_t skip_hi, int64_t nb_active, int64_t d_pad,
                                           int64_t* acc, int grid_blocks, dal_stream_t stream) {
  if (!rows_i8 || !cols_i8 || !acc) return DAL_ERR_ARG;
  if (row_block0 < 0 || n_row_blocks <= 0 || col_block0 < 0 || nb_active <= 0) return DAL_ERR_SHAPE;
  if (j_lo < col_block0 || j_hi < j_lo || j_hi > nb_active || skip_hi < skip_lo) return DAL_ERR_SHAPE;
  if (d_pad <= 0 || d_pad % 128 || d_pad != dal_pad_features(d_pad)) return DAL_ERR_SHAPE;
  if ((row_block0 | n_row_blocks | nb_active) & 1) return DAL_ERR_SHAPE;  // whole 512-row super blocks
  if ((reinterpret_cast<uintptr_t>(rows_i8) | reinterpret_cast<uintptr_t>(cols_i8)) & 15) return DAL_ERR_SHAPE;
  if (j_hi == j_lo || row_block0 >= nb_active) return DAL_OK;
  // (the chunk rule of the fp16 form, by the split operand's bytes)
  const bool small = (j_hi - j_lo) * 256 * d_pad * 4 <= (int64_t{DAL_GRAM_SMALL_MB} << 20);
  return launch_intsym<kFormI8>(rows_i8, row_block0 / 2, n_row_blocks / 2, cols_i8, col_block0, j_lo, j_hi, skip_lo,
                                skip_hi, nb_active / 2, d_pad / 2, static_cast<int>(d_pad / 128), acc, grid_blocks,
                                small ? DAL_GRAM_MIN_CHUNKS_SMALL : DAL_GRAM_MIN_CHUNKS, as_stream(stream));
}

extern "C" int dal_gram_sym_residual_i8(const uint16_t* ops, int64_t nb_active, int64_t row_block0,
                                        int64_t n_row_blocks, int64_t d_pad, int64_t* acc, void* ws, size_t ws_bytes,
                                        dal_stream_t stream) {
  if (d_pad % 128) return DAL_ERR_SHAPE;
  return gram_sym_residual<kFormI8>(ops, nb_active, row_block0, n_row_blocks, d_pad, acc, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------
// The fp4 form (gram_fp4.hpp; pools with d_pad % 256 == 0).
extern "C" int dal_quant_fp4(const uint16_t* ops, int64_t n_rows, int64_t d_pad, uint8_t* out_fp4,
                             dal_stream_t stream) {
  if (!ops || !out_fp4) return DAL_ERR_ARG;
  if (n_rows < 0 || d_pad <= 0 || d_pad % 256 || d_pad != dal_pad_features(d_pad)) return DAL_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(ops) | reinterpret_cast<uintptr_t>(out_fp4)) & 15) return DAL_ERR_SHAPE;
  if (n_rows == 0) return DAL_OK;
  const int64_t n_chunks = n_rows * (d_pad / 32);
  hipLaunchKernelGGL(quant_fp4_kernel, dim3(static_cast<unsigned>(ceil_div(n_chunks, 256))), dim3(256), 0,
                     as_stream(stream), ops, n_chunks, static_cast<int>(d_pad), split_ks(d_pad), out_fp4);
  DAL_RETURN_IF_LAUNCH_FAILED();
  return DAL_OK;
}

extern "C" int dal_gram_rowsum_sym_fp4_skip(const uint8_t* rows_fp4, int64_t row_block0, int64_t n_row_blocks,
                                            const uint8_t* cols_fp4, int64_t col_block0, int64_t j_lo, int64_t j_hi,
                                            int64_t skip_lo, int64_t skip_hi, int64_t nb_active, int64_t d_pad,
                                            int64_t* acc, int grid_blocks, dal_stream_t stream) {
  if (!rows_fp4 || !cols_fp4 || !acc) return DAL_ERR_ARG;
  if (row_block0 < 0 || n_row_blocks <= 0 || col_block0 < 0 || nb_active <= 0) return DAL_ERR_SHAPE;
  if (j_lo < col_block0 || j_hi < j_lo || j_hi > nb_active || skip_hi < skip_lo) return DAL_ERR_SHAPE;
  if (d_pad <= 0 || d_pad % 256 || d_pad != dal_pad_features(d_pad)) return DAL_ERR_SHAPE;
  if ((row_block0 | n_row_blocks | nb_active) & 1) return DAL_ERR_SHAPE;  // whole 512-row super blocks
  if ((reinterpret_cast<uintptr_t>(rows_fp4) | reinterpret_cast<uintptr_t>(cols_fp4)) & 15) return DAL_ERR_SHAPE;
  if (j_hi == j_lo || row_block0 >= nb_active) return DAL_OK;
  // (the chunk rule of the fp16 form, by the split operand's bytes)
  const bool small = (j_hi - j_lo) * 256 * d_pad * 4 <= (int64_t{DAL_GRAM_SMALL_MB} << 20);
  return launch_intsym<kFormFp4>(rows_fp4, row_block0 / 2, n_row_blocks / 2, cols_fp4, col_block0, j_lo, j_hi, skip_lo,
                                 skip_hi, nb_active / 2, d_pad / 4, static_cast<int>(d_pad / 256), acc, grid_blocks,
                                 small ? DAL_GRAM_MIN_CHUNKS_SMALL : DAL_GRAM_MIN_CHUNKS, as_stream(stream));
}

extern "C" int dal_gram_sym_residual_fp4(const uint16_t* ops, int64_t nb_active, int64_t row_block0,
                                         int64_t n_row_blocks, int64_t d_pad, int64_t* acc, void* ws, size_t ws_bytes,
                                         dal_stream_t stream) {
  if (d_pad % 256) return DAL_ERR_SHAPE;
  return gram_sym_residual<kFormFp4>(ops, nb_active, row_block0, n_row_blocks, d_pad, acc, ws, ws_bytes, stream);
}

// The same with launch 1 done by the caller: sigma_h [nb_active / 2][d_pad] and
// s_l [d_pad] as dal_prep_split_fp4 wrote them (read only; the scan and launch
// 3 run, no memset and no sigma pass).
extern "C" int dal_gram_sym_residual_fp4_pre(const uint16_t* ops, int64_t nb_active, int64_t row_block0,
                                             int64_t n_row_blocks, int64_t d_pad, int64_t* acc,
                                             const int64_t* sigma_h, const int64_t* s_l, void* ws, size_t ws_bytes,
                                             dal_stream_t stream) {
  if (d_pad % 256) return DAL_ERR_SHAPE;
  if (!sigma_h || !s_l) return DAL_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(sigma_h) | reinterpret_cast<uintptr_t>(s_l)) & 7) return DAL_ERR_SHAPE;
  return gram_sym_residual<kFormFp4>(ops, nb_active, row_block0, n_row_blocks, d_pad, acc, ws, ws_bytes, stream,
                                     sigma_h, s_l);
}
