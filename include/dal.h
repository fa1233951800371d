/*
 * dal.h -- C ABI of the MI355X-native active-learning query-selection path.
 *
 * Drop-in boundary for the hot path of dv66/Distributed-Active-Learning
 * (final_thesis/uncertainty_sampling.py, density_weighting.py,
 * cosine_similarity.py, similarity.py).  The reference calls Spark MLlib over
 * Py4J for every operation below; each entry point names the reference call
 * site it replaces.  A maintainer binds these with ctypes;
 * the in-tree binding is distributed-active-learning_amd/dal/_lib.py.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Every pointer is DEVICE memory owned by
 *    the caller (the library never allocates); ``stream`` is a hipStream_t
 *    (NULL = default stream) and every call is asynchronous and
 *    stream-ordered.  No global mutable state: calls are re-entrant.
 *  - Return value: DAL_OK (0) or a negative dal_status (argument / shape /
 *    launch errors, detected on the host before or at launch).
 *    Data-dependent conditions found by a kernel (zero-norm row, candidate
 *    overflow) are OR-ed into the caller's device word ``dev_status``
 *    (DAL_FLAG_*), which the caller reads after synchronising.
 *  - Pool rows are fp32, row-major with leading dimension ``ldx`` (floats):
 *    element (i, f) is x[i * ldx + f].  Every entry that takes an ``ldx``
 *    accepts ANY ldx >= d (ldx < d is DAL_ERR_SHAPE, found on the host before
 *    any device call) and an ``x`` that is only 4-byte aligned (8 bytes for
 *    the fp64 rows of DAL_X_F64).  The ldx - d padding elements of a row are
 *    never read as data and never written, nor is anything before x or after
 *    the last row's d-th element.  The outputs are bit-identical for every
 *    stride and every alignment of the same logical matrix: the 16-byte and
 *    LDS-DMA staging of the forest kernels is taken when d % 4 == 0,
 *    ldx % 4 == 0 and x is 16-byte aligned, and 4-byte loads otherwise -- a
 *    matter of speed alone (the rows per block, and with them the row groups
 *    of dal_dw_step's fast level 1, follow the staging; the selection does
 *    not).  The same holds for the ``ld`` (elements) of a bf16 pool, 2-byte
 *    aligned.  The entries that ask for more say so and refuse the rest with
 *    DAL_ERR_SHAPE: dal_kcenter_begin / dal_kcenter_select (ld % 8 == 0 and a
 *    16-byte aligned pool), dal_max_cosine / dal_max_cosine_unit (a
 *    contiguous, 16-byte aligned [n][d] pool: they take no ld), and the
 *    normalised rows ``u`` of dal_gram_rowsum / dal_split_f16 (ld % 4 == 0,
 *    16-byte aligned) -- a library-made buffer, not the caller's pool.
 *    tests/test_gpu_strided_pool.py and tests/test_gpu_strided_bf16.py hold
 *    every such entry to this on poisoned, strided and misaligned pools.
 *  - Normalised pool buffer ``u``: [n_pad][d_pad] fp32, rows padded with zero
 *    rows to dal_pad_rows(n), features padded with zeros to
 *    dal_pad_features(d).  Zero rows/features contribute exactly 0.
 *  - Density accumulator: int64 fixed point, value = acc * 2^-32
 *    (DAL_FIXED_SCALE).  Integer adds are associative, so the density is
 *    bit-identical for any launch geometry and any number of GPUs.
 *  - Sort keys: uint64, smaller = better (dal_score_key() order); NaN scores
 *    map to DAL_KEY_NAN (last), rows that are not candidates to DAL_KEY_NONE.
 *    Ties are broken by the lower global row index.
 */
#ifndef DAL_H
#define DAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dal_stream_t; /* hipStream_t */
typedef void* dal_event_t;  /* hipEvent_t */

enum dal_status {
  DAL_OK = 0,
  DAL_ERR_ARG = -1,         /* null pointer / bad enum */
  DAL_ERR_SHAPE = -2,       /* size, padding or alignment contract violated */
  DAL_ERR_UNSUPPORTED = -3, /* e.g. tree deeper than DAL_MAX_TREE_DEPTH */
  DAL_ERR_HIP = -4,         /* HIP launch / attribute failure */
  DAL_ERR_CAPACITY = -5     /* k or candidate count above the kernel capacity */
};

/* bits OR-ed into *dev_status by kernels */
#define DAL_FLAG_ZERO_NORM 1      /* a pool row has ||x|| == 0 (cosine undefined) */
#define DAL_FLAG_CAND_OVERFLOW 2  /* re-rank candidate set exceeded capacity */
#define DAL_FLAG_RF_SPLITS 4      /* a feature produced more than num_splits + 1 thresholds */
#define DAL_FLAG_SAMPLE_MISS 8    /* fast top-k level 1 over capacity: re-run with level1_passes = 0 */
#define DAL_FLAG_NONFINITE 16     /* dal_scaler_format met a NaN or an infinity */

/* per-row flags (uint8 per pool row) */
#define DAL_ROW_CANDIDATE 1 /* row is in the unlabeled set and may be selected */
#define DAL_ROW_EXCLUDED 2  /* row is in E: dropped from density as i and as j */

#define DAL_DENSITY_NONE 0
#define DAL_DENSITY_FIXED 1
#define DAL_DENSITY_EXACT 2

#define DAL_ASCENDING 0
#define DAL_DESCENDING 1

#define DAL_KEY_NAN 0xFFFFFFFFFFFFFFFEull
#define DAL_KEY_NONE 0xFFFFFFFFFFFFFFFFull
#define DAL_FIXED_SCALE 4294967296.0 /* 2^32 */
#define DAL_ROW_GRANULE 512
#define DAL_CANON_CHUNK 256
#define DAL_MAX_TREE_DEPTH 16
#define DAL_SORT_CAP 8192          /* max pairs the single-block sort handles */
#define DAL_SORT_CAP_PAYLOAD 4096  /* ... when it also carries an fp64 payload */
#define DAL_RF_MAX_SPLITS 255          /* thresholds per feature (bins fit a uint8) */
#define DAL_RF_MAX_SPLIT_SAMPLE 16384  /* rows one threshold search sorts in LDS */
#define DAL_RF_MAX_DEPTH 10            /* deepest tree dal_rf_train grows */
#define DAL_RF_SPLIT_LDS_BYTES 163840  /* m * (num_splits + 2) * classes * 4 must fit (one node's histogram, LDS) */

const char* dal_status_string(int status);
int dal_abi_version(void);
int64_t dal_pad_rows(int64_t n);
int64_t dal_pad_features(int64_t d);
/* Rigorous bound |d_gemm - d_canonical| <= dal_density_error_bound(n_cols)
 * for the fp32-MFMA density ("Density error bound"). */
double dal_density_error_bound(int64_t n_cols);

/* ---- (a1) row L2 normalisation --------------------------------------
 * Replaces density_weighting.py:66 / cosine_similarity.py:28 /
 * similarity.py:28  ``data.map(lambda _: _/np.linalg.norm(_))``.
 * norm64[i] = sqrt(sum_d x_id^2) in fp64 (sequential over d, no FMA);
 * u[i][d] = (float)(x_id / norm64[i]); rows with DAL_ROW_EXCLUDED and rows
 * n..n_pad-1 are written as zeros (E is dropped as j: density_weighting.py:95-100).
 * row_flags may be NULL.  A zero row sets DAL_FLAG_ZERO_NORM. */
int dal_normalize_rows(const float* x, int64_t n, int64_t d, int64_t ldx,
                       const uint8_t* row_flags, int64_t n_pad, int64_t d_pad,
                       float* u, double* norm64, int32_t* dev_status, dal_stream_t stream);

/* OR ``bits`` into flags[idx[t] - row_base] for every index of this shard
 * (0 <= idx - row_base < n): builds DAL_ROW_CANDIDATE from an unlabeled index
 * list without a host round trip. */
int dal_mark_rows(const int64_t* idx, int64_t count, int64_t row_base, int64_t n, int bits,
                  uint8_t* flags, dal_stream_t stream);
/* dal_mark_rows that also writes to *in_range (device int32, zeroed by the
 * call) how many of the count indices fall inside this shard -- the
 * candidate count of a shard given global candidates, with no extra pass
 * (ABI v4). */
int dal_mark_rows_count(const int64_t* idx, int64_t count, int64_t row_base, int64_t n, int bits,
                        uint8_t* flags, int32_t* in_range, dal_stream_t stream);

/* ---- canonical fp64 column sum (re-rank side of the density) -----------
 * partials[c][f] = sum over rows c*256 .. c*256+255 (< n, not EXCLUDED) of
 * x_rf / norm64[r], sequential in row order; rows of a shard start at a
 * multiple of 256.  dal_canon_colsum_reduce sums partials sequentially over c. */
int dal_canon_colsum_partials(const float* x, int64_t n, int64_t d, int64_t ldx,
                              const double* norm64, const uint8_t* row_flags,
                              double* partials, dal_stream_t stream);
int dal_canon_colsum_reduce(const double* partials, int64_t n_chunks, int64_t d,
                            double* colsum, dal_stream_t stream);
/* dal_canon_colsum_partials for the listed chunks only (a new symbol; the ABI
 * number stays): row chunk_ids[b] of the full [ceil(n / 256)][d] partials
 * array is rewritten with the same sequential arithmetic, so it has the bytes
 * a fresh pool with these row_flags produces; every other row is left alone.
 * chunk_ids: device int64 [n_chunks], distinct (an id outside the pool is
 * skipped); n_chunks == 0 launches nothing. */
int dal_canon_colsum_partials_chunks(const float* x, int64_t n, int64_t d, int64_t ldx, const double* norm64,
                                     const uint8_t* row_flags, const int64_t* chunk_ids, int64_t n_chunks,
                                     double* partials, dal_stream_t stream);
/* Separable canonical density (the exact identity sum_j <u_i,u_j> = <u_i, s>):
 * density[i] = sum_f (x_if / norm64[i]) * colsum[f], sequential, no FMA --
 * bit-identical to the re-rank and the oracle; NaN for EXCLUDED rows.
 * O(N*D), HBM-bound; the opt-in alternative to dal_gram_rowsum. */
int dal_density_separable(const float* x, int64_t n, int64_t d, int64_t ldx,
                          const double* norm64, const double* colsum, const uint8_t* row_flags,
                          double* density, dal_stream_t stream);

/* ---- (a2-a4) fused cosine Gram row-sum -------------------------------
 * Replaces density_weighting.py:67-75 (IndexedRowMatrix -> BlockMatrix
 * U.multiply(UT) -> toCoordinateMatrix().entries), :95-100 (L0 exclusion) and
 * :157-161 (groupByKey sum):  acc[i] += sum_j <u_rows[i], u_cols[j]> * 2^32.
 * Tiled fp32 MFMA (v_mfma_f32_32x32x2_f32) with the row-sum fused into the
 * accumulators; S is never materialised.  acc must be zeroed by the caller
 * (the call accumulates, so it can be issued once per column shard).
 * n_rows_pad % 256 == 0, n_cols_pad % 512 == 0, d_pad from dal_pad_features,
 * ld >= d_pad (floats).  grid_blocks <= 0 selects one block per CU. */
int dal_gram_rowsum(const float* u_rows, int64_t n_rows_pad, const float* u_cols,
                    int64_t n_cols_pad, int64_t d_pad, int64_t ld, int64_t* acc,
                    int grid_blocks, dal_stream_t stream);

/* ---- (a2-a4) the same row-sum on fp16 MFMA: symmetric + compensated -------
 * Same replaced reference lines as dal_gram_rowsum, at the fp16 matrix-core
 * rate.  dal_split_f16 writes each normalised fp32 row u (from
 * dal_normalize_rows, ld >= d_pad) at scale 2^12 as H = fp16(2^12 u),
 * L = fp16(2^12 u - H) (RNE) in the layout [n_pad][d_pad / KS][KS H halves |
 * KS L halves], KS = 128 if d_pad % 128 == 0, 32 if d_pad == 32, else 64
 * (dal_split_f16_halves(n_pad, d_pad) halves in all). */
int64_t dal_split_f16_halves(int64_t n_pad, int64_t d_pad);
int dal_split_f16(const float* u, int64_t n_pad, int64_t d_pad, int64_t ld, uint16_t* out,
                  dal_stream_t stream);
/* dal_normalize_rows + dal_split_f16 (one fused kernel) + optionally
 * dal_canon_colsum_partials, same bits (the fp32 unit rows never reach HBM): norm64[i] =
 * canonical ||x_i||, the split operand of the unit rows (E rows, zero-norm
 * rows and padding rows -> zeros) and, if partials != NULL, the canonical
 * column-sum partials [ceil(n / DAL_CANON_CHUNK)][d]; acc_zero (nullable,
 * int64 [n_pad]: the density accumulator the Gram adds into) is zeroed by the
 * same kernel (ABI v3).  n_pad % 512 == 0. */
int dal_prep_split(const float* x, int64_t n, int64_t d, int64_t ldx, const uint8_t* row_flags,
                   int64_t n_pad, int64_t d_pad, uint16_t* out, double* norm64, double* partials,
                   int64_t* acc_zero, int32_t* dev_status, dal_stream_t stream);
/* Symmetric (SYRK-style), compensated Gram row-sum (ABI v5; row sums only
 * since ABI v8).  S = U U^T is symmetric: rows are grouped in 512-row super
 * blocks (pairs of 256-row blocks) and each unordered pair {P, Q} is
 * multiplied once.  P takes Q iff Q == P, or Q > P and P+Q even, or Q < P and
 * P+Q odd (global indices, so the bits do not depend on the sharding).  Both
 * MFMA operands are H only (the L halves of the operand are not read here):
 * per 32 features one v_mfma_f32_16x16x32_f16 forms the row sums of the fp16
 * Gram <H_i, H_j> over the taken pairs (-> acc rows of P).
 * dal_gram_sym_residual adds everything else in closed form: every term with
 * an L factor (<L_i, H_j + L_j> and <H_i, L_j>, over every column j) and the
 * pair's H.H column sums for Q's rows (sum over the P taking Q of <H_j, sum_{i
 * in P} H_i>) -- acc holds the
 * density only after BOTH (any order; integer adds), and each call writes
 * only the acc rows of ITS row blocks (no cross-GPU density sum).  rows: the
 * operand of global 256-row blocks [row_block0, row_block0 + n_row_blocks)
 * (even counts); cols: the operand whose first block is global block
 * col_block0; column blocks [j_lo, j_hi) minus [skip_lo, skip_hi) are
 * processed (j_hi <= nb_active = pad512(N_total) / 256), so a caller can
 * split the columns over several calls.  acc is indexed by GLOBAL row
 * (>= nb_active * 256 entries, zeroed by the caller).  Chains are folded to
 * multiples of 2^-32 and added exactly (int64): the bits do not depend on the
 * grid, the column split or the GPU count.  Rigorous bound on |d -
 * d_canonical| of the completed density: dal_density_error_bound_sym_d. */
int dal_gram_rowsum_sym(const uint16_t* rows, int64_t row_block0, int64_t n_row_blocks,
                        const uint16_t* cols, int64_t col_block0, int64_t j_lo, int64_t j_hi,
                        int64_t nb_active, int64_t d_pad, int64_t* acc, int grid_blocks,
                        dal_stream_t stream);
int dal_gram_rowsum_sym_skip(const uint16_t* rows, int64_t row_block0, int64_t n_row_blocks,
                             const uint16_t* cols, int64_t col_block0, int64_t j_lo, int64_t j_hi,
                             int64_t skip_lo, int64_t skip_hi, int64_t nb_active, int64_t d_pad,
                             int64_t* acc, int grid_blocks, dal_stream_t stream);
/* The closed-form part of dal_gram_rowsum_sym's density for the rows of
 * global blocks [row_block0, row_block0 + n_row_blocks) (even), ADDED into acc
 * (global row index): acc[r] += rint(2^32 * (<L_r, S~> + <H_r, S^L + CH_B>)),
 * B = r's super block, S~ = the sum of H + L and S^L the sum of L over every
 * active row, CH_B = the sum of the H row sums of the other super blocks that
 * take B (their pairs' column sums for B's rows) -- exact int64 sums in units
 * of 2^-24, fp64 dots of products in a fixed order.  ops: the
 * operand of EVERY active row (nb_active * 256 rows: the gathered operand on
 * several GPUs).  Three launches, O(N * D); workspace from
 * dal_gram_sym_residual_workspace_bytes (256-byte aligned). */
size_t dal_gram_sym_residual_workspace_bytes(int64_t nb_active, int64_t n_row_blocks, int64_t d_pad);
int dal_gram_sym_residual(const uint16_t* ops, int64_t nb_active, int64_t row_block0, int64_t n_row_blocks,
                          int64_t d_pad, int64_t* acc, void* ws, size_t ws_bytes, dal_stream_t stream);
/* The int8 form of the same density (pools with d_pad % 128 == 0; new symbols
 * of ABI v10).  With a(h) = clamp(rint(h / 32), -127, 127) of the operand's H
 * terms (dal_quant_i8: [n_rows][d_pad] int8, features in natural order, from
 * the split operand -- a pure function of it) the MFMAs
 * (v_mfma_i32_16x16x64_i8) form the exact int32 row sums of <a_i, a_j> over
 * the taken pairs, and acc receives them times 2^18; dal_gram_sym_residual_i8
 * adds everything else in closed form, decoding every operand element as h' =
 * 32 a(h), l' = (h - h') + l where dal_gram_sym_residual decodes (h, l).  The
 * two belong together: acc holds the density after dal_gram_rowsum_sym_i8_skip
 * AND dal_gram_sym_residual_i8, within the same dal_density_error_bound_sym_d.
 * Arguments as dal_gram_rowsum_sym_skip (rows_i8 / cols_i8: the int8 operands
 * of the same row ranges, 16-byte aligned) and dal_gram_sym_residual (the
 * split operand, the same workspace); always the round-robin schedule. */
int dal_quant_i8(const uint16_t* ops, int64_t n_rows, int64_t d_pad, int8_t* out_i8, dal_stream_t stream);
int dal_gram_rowsum_sym_i8_skip(const int8_t* rows_i8, int64_t row_block0, int64_t n_row_blocks,
                                const int8_t* cols_i8, int64_t col_block0, int64_t j_lo, int64_t j_hi,
                                int64_t skip_lo, int64_t skip_hi, int64_t nb_active, int64_t d_pad, int64_t* acc,
                                int grid_blocks, dal_stream_t stream);
int dal_gram_sym_residual_i8(const uint16_t* ops, int64_t nb_active, int64_t row_block0, int64_t n_row_blocks,
                             int64_t d_pad, int64_t* acc, void* ws, size_t ws_bytes, dal_stream_t stream);
/* The fp4 form of the same density (pools with d_pad % 256 == 0; new symbols,
 * the ABI number stays).  With a4(h) = the element of +-{0, 1, 2, 3, 4, 6, 8, 12}
 * nearest to h / 32 (ties to the smaller magnitude; twice an e2m1 value) of
 * the operand's H terms (dal_quant_fp4: [n_rows][d_pad / 2] bytes of 4-bit
 * e2m1 codes, features in natural order, feature f in byte f / 2, the even
 * one in the low nibble -- a pure function of the split operand) the MFMAs
 * (v_mfma_scale_f32_16x16x128_f8f6f4, fp4 on both sides) form the exact
 * integer row sums of <a4_i, a4_j> over the taken pairs, and acc receives them
 * times 2^18; dal_gram_sym_residual_fp4 adds everything else in closed form,
 * decoding every operand element as h' = 32 a4(h), l' = (h - h') + l.  The two
 * belong together as the int8 pair does, within the same
 * dal_density_error_bound_sym_d.  Arguments as the _i8 pair; always the
 * round-robin schedule. */
int dal_quant_fp4(const uint16_t* ops, int64_t n_rows, int64_t d_pad, uint8_t* out_fp4, dal_stream_t stream);
int dal_gram_rowsum_sym_fp4_skip(const uint8_t* rows_fp4, int64_t row_block0, int64_t n_row_blocks,
                                 const uint8_t* cols_fp4, int64_t col_block0, int64_t j_lo, int64_t j_hi,
                                 int64_t skip_lo, int64_t skip_hi, int64_t nb_active, int64_t d_pad, int64_t* acc,
                                 int grid_blocks, dal_stream_t stream);
int dal_gram_sym_residual_fp4(const uint16_t* ops, int64_t nb_active, int64_t row_block0, int64_t n_row_blocks,
                              int64_t d_pad, int64_t* acc, void* ws, size_t ws_bytes, dal_stream_t stream);
/* The fp4 form's preparation in one pass over the pool (new symbols, the ABI
 * number stays): what dal_prep_split (norm64, the status flag, the zeroed
 * acc_zero, the split operand, the canonical partials), dal_quant_fp4 over
 * all n_pad rows (out_fp4) and launch 1 of dal_gram_sym_residual_fp4 write, the
 * same bytes: sigma_h [n_pad / 512][d_pad] = the sum of h' over each 512-row
 * super block and s_l [d_pad] = the sum of l' over the pool, int64 in units of
 * 2^-24.  One fp64 quotient and one a4 per element.  x_stride: dal_prep_split's
 * ldx (floats between rows, >= d).  d_pad % 256 == 0, n >= 1, n_pad % 512 == 0; partials and acc_zero nullable; ws: scratch of
 * dal_prep_split_fp4_workspace_bytes (8-byte aligned), free once the call's
 * work has run.  dal_gram_sym_residual_fp4_pre is dal_gram_sym_residual_fp4
 * with those sums given (nb_active * 256 == n_pad of the prep call; read
 * only): the scan and the row launch alone. */
size_t dal_prep_split_fp4_workspace_bytes(int64_t n_pad, int64_t d_pad);
int dal_prep_split_fp4(const float* x, int64_t n, int64_t d, int64_t x_stride, const uint8_t* row_flags, int64_t n_pad,
                       int64_t d_pad, uint16_t* out, double* norm64, double* partials, int64_t* acc_zero,
                       uint8_t* out_fp4, int64_t* sigma_h, int64_t* s_l, void* ws, size_t ws_bytes,
                       int32_t* dev_status, dal_stream_t stream);
int dal_gram_sym_residual_fp4_pre(const uint16_t* ops, int64_t nb_active, int64_t row_block0, int64_t n_row_blocks,
                                  int64_t d_pad, int64_t* acc, const int64_t* sigma_h, const int64_t* s_l, void* ws,
                                  size_t ws_bytes, dal_stream_t stream);
double dal_density_error_bound_sym(int64_t n_cols);
/* The same bound for the kernel that runs features padded to d_pad (ABI v8):
 * the row-side chain length charged depends on the slice width KS (1,024
 * products at KS 32, 2,048 at KS 64 / 128: twice what the H.H chains sum, the
 * values are kept and over-charge); dal_density_error_bound_sym(n) ==
 * dal_density_error_bound_sym_d(n, 0) is the longest chain's, valid for any
 * d_pad. */
double dal_density_error_bound_sym_d(int64_t n_cols, int64_t d_pad);

/* ---- density downdate: E grows by a batch Delta --------------------------
 * New symbols only: dal_abi_version() stays 10; a caller probes for
 * dal_density_downdate (absent from older libraries).
 * The usual information density sums over the CURRENT unlabeled pool, so a
 * row leaves every density when it is labeled (the reference freezes E at L0,
 * density_weighting.py:95-100).  Growing E by Delta (m rows) lowers each
 * density by sum_{j in Delta} <u_i, u_j>: an N x m product, not a new Gram.
 *   acc[i] -= fixed(sum_{j < m} <u_i, u_j>)   for every row i of ops
 * ops: the split operand (dal_split_f16's layout) of the rows acc belongs to,
 * [n_pad][2 * d_pad], n_pad % 256 == 0; delta_ops: the operand rows of Delta
 * in the same layout, [m_pad][2 * d_pad] with m_pad = m rounded up to
 * DAL_DOWNDATE_TILE and rows m .. m_pad - 1 zero, gathered BEFORE those rows
 * are zeroed in ops; both 16-byte aligned.  acc: int64 [n_pad] fixed point
 * (x 2^32), updated in place, one owner per row, chains folded to multiples
 * of 2^-32 and subtracted as integers: its bytes do not depend on grid_blocks
 * (<= 0: two blocks per CU) or on the run.  fp16 MFMA on H.H + H.L + L.H of
 * the split (L.L is charged to the bound); every form of the "sym" Gram
 * (fp16, int8, fp4) keeps this operand, so there is one downdate.
 * Contract: if acc held the density of E within a bound B, it holds the
 * density of E u Delta within B + dal_density_downdate_error_bound(m, d_pad)
 * on every row outside E u Delta (rigorous, non-decreasing in m; DESIGN.md,
 * "Density downdate").  The caller then repairs what else is keyed by E: the
 * row flags, the operand rows of Delta (zeros) and the column-sum partials
 * (dal_canon_colsum_partials_chunks).
 * Null pointer or misaligned operand DAL_ERR_ARG; n_pad % 256, a d_pad not
 * from dal_pad_features or m < 1 DAL_ERR_SHAPE; m > DAL_DOWNDATE_MAX_ROWS
 * DAL_ERR_CAPACITY (the caller chunks a longer Delta). */
#define DAL_DOWNDATE_MAX_ROWS 1024
#define DAL_DOWNDATE_TILE 64
double dal_density_downdate_error_bound(int64_t m, int64_t d_pad);
int dal_density_downdate(const uint16_t* ops, int64_t n_pad, int64_t d_pad, const uint16_t* delta_ops, int64_t m,
                         int64_t* acc, int grid_blocks, dal_stream_t stream);

/* ---- (a5-a10) forest votes + uncertainty / density-weighted score ------
 * Replaces uncertainty_sampling.py:88-98 / density_weighting.py:136-167:
 * T x DecisionTreeModel.predict, groupByKey vote sum, the LUT score and the
 * e*d product.  Forest in complete-heap SoA layout (dal/forest.py):
 *   inner[t][h] = {feature (int32), threshold bits (fp32, rounded toward -inf
 *   from fp64 so that x32 <= t32  <=>  x <= t64)}, h < 2^depth - 1,
 *   leaf[t][l] in {0,1}, l < 2^depth.  x[f] <= thr -> child 2h+1, else 2h+2.
 * lut: fp64[T+1].  density_kind 0 (density NULL) -> uncertainty mode:
 * score = lut[v]; else score = lut[v] * d^beta (NaN for EXCLUDED rows) with
 * d = ((int64*)density)[i] * 2^-32 (kind DAL_DENSITY_FIXED, the GEMM
 * accumulator; interval scores) or d = ((double*)density)[i] (kind
 * DAL_DENSITY_EXACT, canonical fp64; exact scores, keys_hi == keys).
 * keys[i] = dal score key for ``order`` (DAL_KEY_NONE when not CANDIDATE).
 * In density mode the GEMM density is approximate, so each score is an
 * interval [score - err_i, score + err_i], err_i = |lut[v]| * density_err
 * (beta = 1; the d^beta image of the interval otherwise): keys[i] is the
 * PESSIMISTIC end's key and keys_hi[i] (nullable) the OPTIMISTIC end's key;
 * exact scores (lut[v] == 0 or NaN) have keys[i] == keys_hi[i]. */
int dal_forest_score(const float* x, int64_t n, int64_t d, int64_t ldx,
                     const int32_t* inner, const uint8_t* leaf, int32_t n_trees, int32_t depth,
                     const double* lut, const void* density, int density_kind, double density_err,
                     const uint8_t* row_flags, double beta, int order,
                     int32_t* votes, double* scores, uint64_t* keys, uint64_t* keys_hi,
                     dal_stream_t stream);

/* ---- (a5-a10) the same over the pool's blocked feature-major copy (ABI v9)
 * dal_pool_blocked writes the pool as tiles of 64 rows, feature-major inside
 * a tile: xb[(t * d + f) * 64 + r] = x[t * 64 + r][f], rows past n zero
 * (dal_pool_blocked_floats(n, d) floats; a per-pool copy, built once -- the
 * pool is constant across AL iterations).  dal_forest_score_blocked gives
 * dal_forest_score's outputs bit for bit; when dal_forest_blocked_rows(d,
 * n_trees, depth) is non-zero (the forest's node count bounds its distinct
 * features at <= 256, and a tile of those plus the forest fits 96 KiB of LDS)
 * it reads only the features the forest tests -- each tile's listed features
 * as 256-B runs (config 4, T = 10: ~116 of 256 features) -- else it runs
 * dal_forest_score's row-major kernel on x.  xb must be 16-B aligned.
 * Every inner node's feature must lie in [0, d) (the forest is device data, so
 * the library does not read it back to check; dal.forest.Forest.check_features
 * does before upload).  For an invalid forest the outputs are unspecified and
 * the two entry points differ: the blocked kernel clamps a feature into
 * [0, d - 1], the row-major kernel does not. */
int dal_forest_blocked_rows(int64_t d, int32_t n_trees, int32_t depth);
int64_t dal_pool_blocked_floats(int64_t n, int64_t d);
int dal_pool_blocked(const float* x, int64_t n, int64_t d, int64_t ldx, float* xb, dal_stream_t stream);
/* The prepared forest (ABI v10): the blocked kernel's per-block forest setup
 * (the distinct tested features, every node's feature remapped to its slot in
 * that list, the leaves) done ONCE per (forest, d) into a caller-owned device
 * buffer of dal_forest_prep_bytes(d, n_trees, depth) bytes (16-B aligned; 0
 * when dal_forest_blocked_rows is 0).  Pass it as ``fprep`` to
 * dal_forest_score_blocked / dal_dw_step / dal_dw_plan_create with the same
 * forest (inner, leaf, n_trees, depth) and d: each block of the score kernel
 * then copies it into LDS instead of rebuilding it; the outputs are the same
 * bits.  A stale fprep (another forest) gives that forest's votes: re-prepare
 * after the forest changes (stream-ordered: one launch, one block).  Reads the
 * forest arrays; a node feature outside [0, d) is clamped (as the unprepared
 * blocked kernel does) and counted in the buffer's second int32 word. */
size_t dal_forest_prep_bytes(int64_t d, int32_t n_trees, int32_t depth);
int dal_forest_prepare(const int32_t* inner, const uint8_t* leaf, int32_t n_trees, int32_t depth, int64_t d,
                       void* fprep, size_t fprep_bytes, dal_stream_t stream);
int dal_forest_score_blocked(const float* x, const float* xb, const void* fprep, int64_t n, int64_t d,
                             int64_t ldx, const int32_t* inner, const uint8_t* leaf, int32_t n_trees,
                             int32_t depth, const double* lut, const void* density, int density_kind,
                             double density_err, const uint8_t* row_flags, double beta, int order,
                             int32_t* votes, double* scores, uint64_t* keys, uint64_t* keys_hi,
                             dal_stream_t stream);

/* ---- (a5-a10, C classes) per-class forest votes + uncertainty score ------
 * New symbols only: dal_abi_version() stays 10, and a caller probes for the
 * feature with dal_forest_multiclass_max_classes() (32; absent from older
 * libraries).  The forest is dal_forest_score's complete-heap SoA with leaf
 * bytes holding class ids in {0..n_classes-1}, 2 <= n_classes <= 32,
 * 1 <= n_trees <= 255.  n_c(i) = the number of trees whose leaf for row i is
 * class c (sum_c n_c = T); counts[i][c] = n_c(i) (nullable), pred[i] = the
 * smallest c with maximal n_c (nullable).  lut: fp64[T+1] (dal.luts.
 * multiclass_lut), and by score_kind
 *   DAL_MC_LEAST_CONFIDENCE  scores[i] = lut[max_c n_c]
 *   DAL_MC_MARGIN            scores[i] = lut[n_(1) - n_(2)], largest minus
 *                            second-largest count (integer subtraction)
 *   DAL_MC_ENTROPY           scores[i] = ((0.0 + lut[n_0]) + lut[n_1]) + ...,
 *                            sequential fp64 adds in class order
 * keys[i] = the score key for ``order``, DAL_KEY_NONE when the row is not
 * DAL_ROW_CANDIDATE (row_flags NULL: every row is a candidate); select with
 * dal_topk.  A leaf byte >= n_classes is counted for no class (the forest is
 * device data and is not read back; dal.forest.Forest.check_classes checks it
 * before upload).  Uncertainty only, on the row-major pool: the density form
 * and the forms over the blocked copy follow; no plan. */
#define DAL_MC_MAX_CLASSES 32
#define DAL_MC_MAX_TREES 255
#define DAL_MC_LEAST_CONFIDENCE 0
#define DAL_MC_MARGIN 1
#define DAL_MC_ENTROPY 2
int dal_forest_multiclass_max_classes(void);
int dal_forest_score_multiclass(const float* x, int64_t n, int64_t d, int64_t ldx,
                                const int32_t* inner, const uint8_t* leaf, int32_t n_trees, int32_t depth,
                                int32_t n_classes, const double* lut, int score_kind,
                                const uint8_t* row_flags, int order, uint8_t* counts, uint8_t* pred,
                                double* scores, uint64_t* keys, dal_stream_t stream);

/* ---- (a5-a10, C classes) class entropy x density^beta, interval keys -----
 * The C-class reading of density_weighting.py:148-167's e*d product (a new
 * definition: the reference's one-sided -(1-p) log2(1-p) has no C-class form;
 * at n_classes = 2 this is the two-term Shannon entropy).  A new symbol only:
 * dal_abi_version() stays 10.  Forest, counts and pred as
 * dal_forest_score_multiclass; lut = dal.luts.multiclass_lut("entropy", T):
 *   entropy[i]   = ((0.0 + lut[n_0]) + lut[n_1]) + ...   class order, >= +0.0
 *   scores[i]    = entropy[i] * d_i^beta   (one fp64 multiply, no FMA; d_i^beta
 *                  = d_i at beta == 1), NaN for DAL_ROW_EXCLUDED rows
 *   row_index[i] = i   (int32: n <= INT32_MAX, else DAL_ERR_SHAPE)
 * d_i and the keys as dal_forest_score's density mode, always descending:
 * density_kind DAL_DENSITY_FIXED ((int64*)density)[i] * 2^-32, the GEMM
 * accumulator, |d - d_canonical| <= density_err: keys[i] is the key of the
 * pessimistic end scores[i] - err_i, keys_hi[i] (nullable) of the optimistic
 * end scores[i] + err_i, err_i = entropy[i] * density_err at beta == 1 (the
 * d^beta image of the interval otherwise), floored at |scores[i]| * 4.5e-16;
 * DAL_DENSITY_EXACT ((double*)density)[i], canonical fp64: keys_hi == keys.
 * Point intervals (entropy 0, NaN) have keys_hi == keys; rows that are not
 * DAL_ROW_CANDIDATE (row_flags NULL: every row is one) get DAL_KEY_NONE in
 * both.  The exact selection is dal_dw_select unchanged, with votes =
 * row_index and lut = entropy: its re-rank then forms entropy[i] *
 * (canonical density)^beta.  n == 0 returns DAL_OK before any device call. */
int dal_forest_score_multiclass_dw(const float* x, int64_t n, int64_t d, int64_t ldx,
                                   const int32_t* inner, const uint8_t* leaf, int32_t n_trees, int32_t depth,
                                   int32_t n_classes, const double* lut, const void* density,
                                   int density_kind, double density_err, const uint8_t* row_flags, double beta,
                                   uint8_t* counts, uint8_t* pred, double* entropy, int32_t* row_index,
                                   double* scores, uint64_t* keys, uint64_t* keys_hi, dal_stream_t stream);

/* ---- (a5-a10, C classes) the same two over the pool's blocked copy -------
 * New symbols only: dal_abi_version() stays 10, and a caller probes for the
 * feature with dal_forest_multiclass_blocked_rows (absent from older
 * libraries).  xb is dal_pool_blocked's copy of x and fprep dal_forest_prepare's
 * buffer for the same forest (inner, leaf, n_trees, depth) and d, both
 * unchanged: one prepared buffer per (forest, d) serves dal_forest_score_blocked
 * and these entries (it carries the leaf bytes verbatim, so the class ids).
 * dal_forest_multiclass_blocked_rows is pure host code: 64 (the rows per tile)
 * when the C-class blocked kernel applies, else 0.  It applies when
 * dal_forest_blocked_rows(d, n_trees, depth) is non-zero (a prepared forest
 * exists), 2 <= n_classes <= 32, 1 <= n_trees <= 255, and the block's LDS --
 * the tile of min(nodes, d) 256-B runs, the prepared payload, the score table
 * and the cross-wave exchange of the packed counts ((waves - 1) * ceil4(C) / 4
 * words per row, 4 or 8 waves) -- stays within 96 KiB.
 * dal_forest_score_multiclass_blocked / dal_forest_score_multiclass_dw_blocked
 * take x, xb, fprep and then dal_forest_score_multiclass's /
 * dal_forest_score_multiclass_dw's arguments from n on, and give those
 * entries' outputs bit for bit (counts, pred, scores, keys; and counts, pred,
 * entropy, row_index, scores, keys, keys_hi), reading only the features the
 * forest tests.  xb == NULL runs the row-major kernel on x (fprep ignored).
 * Otherwise xb must be 16-B aligned; when the rule above gives 0 the row-major
 * kernel runs on x, same bits, fprep ignored; when it gives 64, fprep must be
 * non-NULL and 16-B aligned (there is no unprepared form) -- anything else is
 * DAL_ERR_ARG.  Every other check and status is the row-major entry's: n == 0
 * returns DAL_OK before any device call, n > INT32_MAX is DAL_ERR_SHAPE for
 * the density-weighted form.  A leaf byte >= n_classes is counted for no
 * class; rows past n in the last tile are never written.  A stale fprep
 * (another forest) gives that forest's votes.  Every inner node's feature must
 * lie in [0, d): for an invalid forest the outputs are unspecified (the
 * prepared forest clamps, the row-major kernel does not).  Selection is
 * dal_topk / dal_dw_select after these entries; the fused step with the group
 * minima folded by the score kernel, and its plan, are dal_dw_step_multiclass
 * and dal_dw_plan_create_multiclass below. */
int dal_forest_multiclass_blocked_rows(int64_t d, int32_t n_trees, int32_t depth, int32_t n_classes);
int dal_forest_score_multiclass_blocked(const float* x, const float* xb, const void* fprep, int64_t n, int64_t d,
                                        int64_t ldx, const int32_t* inner, const uint8_t* leaf, int32_t n_trees,
                                        int32_t depth, int32_t n_classes, const double* lut, int score_kind,
                                        const uint8_t* row_flags, int order, uint8_t* counts, uint8_t* pred,
                                        double* scores, uint64_t* keys, dal_stream_t stream);
int dal_forest_score_multiclass_dw_blocked(const float* x, const float* xb, const void* fprep, int64_t n, int64_t d,
                                           int64_t ldx, const int32_t* inner, const uint8_t* leaf,
                                           int32_t n_trees, int32_t depth, int32_t n_classes, const double* lut,
                                           const void* density, int density_kind, double density_err,
                                           const uint8_t* row_flags, double beta, uint8_t* counts, uint8_t* pred,
                                           double* entropy, int32_t* row_index, double* scores, uint64_t* keys,
                                           uint64_t* keys_hi, dal_stream_t stream);

/* ---- soft votes: averaged leaf class distributions, exact ----------------
 * New symbols only: dal_abi_version() stays 10, and a caller probes for the
 * feature with dal_forest_soft_max_depth() (DAL_SOFT_MAX_DEPTH; absent from
 * older libraries).  The uncertainty of scikit-learn's predict_proba (modAL's
 * uncertainty, margin and entropy sampling; spark.ml's probabilityCol): a tree
 * contributes its leaf's class distribution, not one class id.
 *
 * The forest: inner is dal_forest_score's complete heap (int32 [T][2^D - 1][2],
 * feature and fp32 threshold bits, x[f] <= thr goes left); leaf_id
 * (int32 [T][2^D]) names, for every heap leaf, a row of the leaf table leaf_q
 * (uint32 [n_leaves][n_classes]); leaf_q[l][c] = rint(p_l[c] 2^31), the
 * leaf's class distribution in fixed point (<= DAL_SOFT_ONE; a row's words
 * need not sum to DAL_SOFT_ONE).  1 <= n_trees <= 255, 2 <= n_classes <= 32,
 * 1 <= depth <= DAL_SOFT_MAX_DEPTH.
 *
 *   S_c(i)   = sum_t leaf_q[leaf_id[t][leaf_t(x_i)]][c]   exact, < 2^39
 *   sums[i][c] = S_c(i) (nullable);  pred[i] = the smallest c with maximal S_c
 *   (nullable);  with M = n_trees 2^31 and by score_kind
 *   DAL_SOFT_LEAST_CONFIDENCE  scores[i] = (double)max_c S_c / (double)M
 *   DAL_SOFT_MARGIN            scores[i] = (double)(S_(1) - S_(2)) / (double)M,
 *                              largest minus second largest, an integer
 *                              difference, then the one division
 *   DAL_SOFT_ENTROPY           scores[i] = ((0.0 + h(p_0)) + h(p_1)) + ...,
 *                              p_c = (double)S_c / (double)M, h(p) = -p log2(p),
 *                              h(0) = +0.0; sequential fp64 adds in class order,
 *                              no FMA; never NaN or -0.0
 * Every division is the IEEE one, so sums, pred and the first two scores are
 * the same bits for every launch shape and on every device; the entropy
 * carries the device log2's error (within n_classes 2^-49 of the host's).
 * keys[i] = the score key for ``order``, DAL_KEY_NONE when the row is not
 * DAL_ROW_CANDIDATE (row_flags NULL: every row is a candidate); select with
 * dal_topk.
 *
 * x_stride is the row stride of x in elements, with the semantics of the other
 * entries' ldx: any x_stride >= d and any 4-byte alignment of x (16-byte
 * aligned rows with d % 4 == 0 take the wider staging forms).
 * Before any device call: a null x, inner, leaf_id, leaf_q, scores or keys, or
 * a bad order or score_kind, is DAL_ERR_ARG; then n < 0, d < 1, d > 2^30,
 * x_stride < d, n_leaves < 1 or n_leaves > 2^26 DAL_ERR_SHAPE; then a depth,
 * n_classes or n_trees outside the limits DAL_ERR_UNSUPPORTED.  n == 0 returns
 * DAL_OK and launches nothing.  A leaf_id outside [0, n_leaves) is the caller's
 * error (dal.forest.ProbabilityForest checks it before upload): the kernel
 * clamps it into the table.  Every inner node's feature must lie in [0, d). */
#define DAL_SOFT_MAX_DEPTH 16
#define DAL_SOFT_MAX_CLASSES 32
#define DAL_SOFT_MAX_TREES 255
#define DAL_SOFT_ONE 2147483648u
#define DAL_SOFT_LEAST_CONFIDENCE 0
#define DAL_SOFT_MARGIN 1
#define DAL_SOFT_ENTROPY 2
int dal_forest_soft_max_depth(void);
int dal_forest_score_soft(const float* x, int64_t n, int64_t d, int64_t x_stride, const int32_t* inner,
                          const int32_t* leaf_id, const uint32_t* leaf_q, int64_t n_leaves, int32_t n_trees,
                          int32_t depth, int32_t n_classes, int score_kind, const uint8_t* row_flags, int order,
                          uint64_t* sums, uint8_t* pred, double* scores, uint64_t* keys, dal_stream_t stream);

/* ---- soft votes: class entropy x density^beta, interval keys --------------
 * modAL's information density on predict_proba: entropy(predict_proba) *
 * density^beta.  New symbols only: dal_abi_version() stays 10, and a caller
 * probes for the symbol (absent from older libraries).  Forest, x_stride, sums
 * and pred as dal_forest_score_soft; the kind is DAL_SOFT_ENTROPY and the
 * order descending:
 *   entropy[i]   = dal_forest_score_soft(DAL_SOFT_ENTROPY)'s scores[i], the
 *                  same bits (>= +0.0, never NaN; within n_classes 2^-49 of
 *                  the host's entropy of S_c / M)
 *   scores[i]    = entropy[i] * d_i^beta   (one fp64 multiply, no FMA; d_i^beta
 *                  = d_i at beta == 1), NaN for DAL_ROW_EXCLUDED rows
 *   row_index[i] = i   (int32: n <= INT32_MAX, else DAL_ERR_SHAPE)
 * d_i, density_kind, density_err, keys, keys_hi (nullable) and the candidates'
 * DAL_KEY_NONE exactly as dal_forest_score_multiclass_dw: with
 * DAL_DENSITY_FIXED keys[i] / keys_hi[i] are the keys of scores[i] -+ err_i,
 * err_i = entropy[i] * density_err at beta == 1 (the d^beta image of the
 * interval otherwise), floored at |scores[i]| * 4.5e-16 and zero where
 * entropy[i] == 0 or the row is excluded; with DAL_DENSITY_EXACT keys_hi ==
 * keys.  Exactness is therefore stated on the entropy the call returned: for
 * every candidate outside the excluded set, keys_hi <= key(entropy[i] *
 * d_canonical^beta) <= keys.  The exact selection is dal_dw_select unchanged,
 * with votes = row_index and lut = entropy.
 * Before any device call: a null x, inner, leaf_id, leaf_q, density, entropy,
 * row_index, scores or keys, or a bad density_kind, is DAL_ERR_ARG; then
 * dal_forest_score_soft's DAL_ERR_SHAPE conditions and n > INT32_MAX; then its
 * DAL_ERR_UNSUPPORTED ones.  n == 0 returns DAL_OK and launches nothing. */
int dal_forest_score_soft_dw(const float* x, int64_t n, int64_t d, int64_t x_stride, const int32_t* inner,
                             const int32_t* leaf_id, const uint32_t* leaf_q, int64_t n_leaves, int32_t n_trees,
                             int32_t depth, int32_t n_classes, const void* density, int density_kind,
                             double density_err, const uint8_t* row_flags, double beta, uint64_t* sums,
                             uint8_t* pred, double* entropy, int32_t* row_index, double* scores, uint64_t* keys,
                             uint64_t* keys_hi, dal_stream_t stream);

/* ---- soft votes: BALD, the trees' mutual information ----------------------
 * Query by committee on the leaf distributions: the mean KL divergence of the
 * trees' distributions p_t to their average,
 *   (1/T) sum_t KL(p_t || pbar) = H(pbar) - (1/T) sum_t H(p_t)
 * (BALD; the committee's Jensen-Shannon divergence; modAL's KL disagreement).
 * A new symbol only: dal_abi_version() stays 10, and a caller probes for the
 * symbol (absent from older libraries).  Forest, x_stride, sums, pred, keys
 * and the candidates' DAL_KEY_NONE as dal_forest_score_soft.
 *
 * leaf_h (uint32 [n_leaves]) holds every leaf's entropy in fixed point,
 *   leaf_h[l] = rint(H_l 2^DAL_SOFT_ENTROPY_SHIFT),
 *   H_l = ((0.0 + h(q[l][0] / 2^31)) + h(q[l][1] / 2^31)) + ..., h as above
 * (H_l <= log2(32) = 5 and 5 2^29 < 2^32; dal.forest.ProbabilityForest.leaf_h
 * computes the words on the host).  The call is defined on the words it is
 * given:
 *   hsum[i]    = sum_t leaf_h[leaf_id[t][leaf_t(x_i)]]    exact, < 2^41 (nullable)
 *   entropy[i] = dal_forest_score_soft(DAL_SOFT_ENTROPY)'s scores[i], the same
 *                bits (nullable)
 *   g          = (double)hsum[i] / (double)(n_trees 2^29), one IEEE division of
 *                two exactly representable integers
 *   b          = entropy[i] - g, one rounding, no FMA
 *   scores[i]  = b > 0 ? b : +0.0     never negative, -0.0 or NaN
 * In real arithmetic b >= 0 (-p log p is concave); the clamp removes what the
 * 2^-30 word rounding and the fp64 log2 can push below zero.  scores are
 * within (n_classes + 1) 2^-49 of the host's evaluation of the same words.
 * ``order`` keys the scores (DAL_DESCENDING selects the largest disagreement).
 * Before any device call: a null x, inner, leaf_id, leaf_q, leaf_h, scores or
 * keys, or a bad order, is DAL_ERR_ARG; then dal_forest_score_soft's
 * DAL_ERR_SHAPE and DAL_ERR_UNSUPPORTED conditions, in its order.  n == 0
 * returns DAL_OK and launches nothing. */
#define DAL_SOFT_ENTROPY_SHIFT 29
int dal_forest_score_soft_bald(const float* x, int64_t n, int64_t d, int64_t x_stride, const int32_t* inner,
                               const int32_t* leaf_id, const uint32_t* leaf_q, const uint32_t* leaf_h,
                               int64_t n_leaves, int32_t n_trees, int32_t depth, int32_t n_classes,
                               const uint8_t* row_flags, int order, uint64_t* sums, uint8_t* pred, uint64_t* hsum,
                               double* entropy, double* scores, uint64_t* keys, dal_stream_t stream);

/* ---- (a11) top-k: sortBy(score).take(k) --------------------------------
 * Replaces uncertainty_sampling.py:106,109 / density_weighting.py:168,172.
 * The k smallest keys, ties -> lower index; out_idx = idx_base + row, sorted
 * by (key, index).  1 <= k <= min(n, DAL_SORT_CAP).  Exact radix select
 * (8 x 8-bit digit histograms) + ordered compaction + one-block bitonic sort. */
size_t dal_topk_workspace_bytes(int64_t n, int64_t k);
int dal_topk(const uint64_t* keys, int64_t n, int64_t k, int64_t idx_base, void* ws,
             size_t ws_bytes, int64_t* out_idx, uint64_t* out_keys, dal_stream_t stream);

/* ---- density-weighted selection with exact fp64 re-rank ----------------
 * Given the interval keys written by dal_forest_score (density mode,
 * DAL_DESCENDING): K = k-th smallest pessimistic key; candidates = every row
 * whose optimistic key is < K (or == K with a non-point interval) plus the
 * first k point-interval rows == K, in row order -- a superset of the
 * canonical top-k (at most ``cap`` of them).  Each candidate's canonical fp64
 * score  lut[v] * (sum_f (x_if / norm64[i]) * colsum[f])^beta  (sequential,
 * no FMA; beta == 2 is one multiply, the correctly rounded square, any other
 * beta != 1 the device pow, good to an ulp) is recomputed and an exact top-k over the candidates returns the k
 * best by (score desc, NaN last, index asc): bit-exact with the fp64 oracle.
 * out_scores are canonical fp64 scores, out_keys (nullable) their keys.  More
 * than ``cap`` candidates sets DAL_FLAG_CAND_OVERFLOW (retry with a larger cap).
 * colsum_ready (nullable): an event recorded after ``colsum`` was written on
 * another stream; the call makes ``stream`` wait for it just before the
 * re-rank (the radix select and compaction run without it), so a cold step's
 * canonical column sum overlaps the candidate search.
 * level1_passes > 0 (1..5; cap <= DAL_SORT_CAP_PAYLOAD): the fast level 1
 * (ABI v6) -- the pool is cut into <= 4096 row groups, tau = the k-th smallest
 * group-minimum pessimistic key (k keys of the pool, so tau >= K), and the
 * candidates are every row whose optimistic key is <= tau, found by scanning
 * only the groups whose minimum optimistic key is <= tau: a superset of the
 * exact candidates in two launches (group minima; tau + append with the
 * in-place canonical re-rank + the final sort by the block that finishes
 * last).  More than cap candidates sets DAL_FLAG_SAMPLE_MISS: re-run with
 * level1_passes = 0.  The selection is the same either way. */
size_t dal_dw_select_workspace_bytes(int64_t n, int64_t k, int64_t cap);
int dal_dw_select(const uint64_t* keys_lo, const uint64_t* keys_hi, const int32_t* votes,
                  const uint8_t* row_flags, int64_t n, int64_t k, int64_t idx_base,
                  const double* lut, double beta, const float* x, int64_t d, int64_t ldx,
                  const double* norm64, const double* colsum, int64_t cap, int32_t level1_passes, void* ws,
                  size_t ws_bytes, int64_t* out_idx, double* out_scores, uint64_t* out_keys,
                  int32_t* dev_status, dal_event_t colsum_ready, dal_stream_t stream);

/* ---- one density-weighted iteration in one call (a5-a11) ----------------
 * The body of density_weighting.py:133-176 for a cached density: equivalent to
 * dal_forest_score(x, ..., density_fixed, DAL_DENSITY_FIXED, density_err,
 * row_flags, beta, DAL_DESCENDING, votes, scores, keys_lo, keys_hi) followed by
 * dal_dw_select(keys_lo, keys_hi, votes, row_flags, n, k, idx_base, lut, beta,
 * x, d, ldx, norm64, colsum, cap, level1_passes, ...) -- same outputs, same
 * bits -- with the fast level 1 fused when level1_passes > 0 (and cap <=
 * DAL_SORT_CAP_PAYLOAD): the score kernel folds each block's minimum keys
 * into the row groups itself, and ONE more launch derives tau, appends the
 * candidates with their canonical scores and sorts them (capacity check:
 * DAL_FLAG_SAMPLE_MISS; the level-1 words are cleared for the next call).
 * step_flags:
 *   DAL_STEP_RESET_STATUS  *dev_status is zeroed at the start of the step (on
 *                          the device: a replayed hipGraph needs no memset node);
 *   DAL_STEP_WS_CLEAN      the workspace header is zero on entry (a previous
 *                          dal_dw_step left it so, or the caller zeroed the
 *                          workspace once): no zeroing launch.  The header is
 *                          left zero on exit whenever this flag is given.
 *   DAL_STEP_KEEP_GROUPS   (ABI v8; MEASUREMENT flag, fast level 1) the row-group
 *                          minima the step folded are left in the workspace
 *                          instead of cleared, so that DAL_STEP_SELECT_ONLY
 *                          calls can re-run the selection.  The workspace is
 *                          then NOT clean for a full step: the next call on it
 *                          MUST be DAL_STEP_SELECT_ONLY, and the sequence ends
 *                          with a SELECT_ONLY call without KEEP_GROUPS (which
 *                          clears the minima) before any full step uses the
 *                          workspace with DAL_STEP_WS_CLEAN again.
 *   DAL_STEP_SELECT_ONLY   (ABI v8; MEASUREMENT flag; with DAL_STEP_WS_CLEAN, fast
 *                          level 1, no DAL_STEP_RESET_STATUS) only the selection
 *                          launch: it re-reads the votes, keys and group minima
 *                          that the previous call with DAL_STEP_KEEP_GROUPS left
 *                          on the same buffers and workspace (the same
 *                          arguments), and gives the same outputs.  bench.py
 *                          times the fused step's selection launch on its own
 *                          with these two flags (time_step_select); the product
 *                          path never sets them.
 * xb (ABI v9; nullable): the pool's blocked copy (dal_pool_blocked) -- the
 * score kernel is then dal_forest_score_blocked's; fprep (ABI v10; nullable,
 * with xb): the forest prepared by dal_forest_prepare.
 * Workspace: dal_dw_step_workspace_bytes (== dal_dw_select's). */
#define DAL_STEP_RESET_STATUS 1u
#define DAL_STEP_WS_CLEAN 2u
#define DAL_STEP_KEEP_GROUPS 4u
#define DAL_STEP_SELECT_ONLY 8u
size_t dal_dw_step_workspace_bytes(int64_t n, int64_t k, int64_t cap);
int dal_dw_step(const float* x, const float* xb, const void* fprep, int64_t n, int64_t d, int64_t ldx,
                const int32_t* inner,
                const uint8_t* leaf,
                int32_t n_trees, int32_t depth, const double* lut, const int64_t* density_fixed,
                double density_err, const uint8_t* row_flags, double beta, int64_t idx_base,
                const double* norm64, const double* colsum, int64_t k, int64_t cap, int32_t level1_passes,
                uint32_t step_flags, void* ws, size_t ws_bytes, int32_t* votes, double* scores,
                uint64_t* keys_lo, uint64_t* keys_hi, int64_t* out_idx, double* out_scores,
                uint64_t* out_keys, int32_t* dev_status, dal_event_t colsum_ready, dal_stream_t stream);

/* ---- one density-weighted iteration over a C-class forest in one call ----
 * New symbols only: dal_abi_version() stays 10; a caller probes for the
 * feature with dal_dw_step_multiclass_form (absent from older libraries).
 * dal_dw_step_multiclass is equivalent to dal_forest_score_multiclass_dw_blocked
 * (x, xb, fprep, ..., lut, density_fixed, DAL_DENSITY_FIXED, density_err,
 * row_flags, beta, counts, pred, entropy, row_index, scores, keys_lo, keys_hi)
 * followed by dal_dw_select(keys_lo, keys_hi, row_index, row_flags, n, k,
 * idx_base, entropy, beta, x, d, ldx, norm64, colsum, cap, level1_passes, ...)
 * -- same outputs, same bits -- as dal_dw_step is to the binary pair: with the
 * fast level 1 the blocked C-class kernel folds each tile's minimum keys into
 * the row groups itself when the pool has at least 2k tiles (else, and with the
 * row-major kernel, one group-minimum pass follows the score kernel), and ONE
 * more launch derives tau, appends the candidates with their canonical scores
 * and sorts them.  lut is multiclass_lut("entropy", T): T + 1 doubles.
 * step_flags: DAL_STEP_RESET_STATUS and DAL_STEP_WS_CLEAN as for dal_dw_step;
 * the two measurement flags are DAL_ERR_ARG.  counts and pred are nullable.
 * xb (nullable) and fprep: as dal_forest_score_multiclass_dw_blocked's, with
 * every check of that entry (2 <= n_classes <= 32, n_trees <= 255, n <=
 * INT32_MAX, 16-B aligned xb, fprep present and aligned where
 * dal_forest_multiclass_blocked_rows gives 64); n == 0 returns DAL_OK before the
 * selection's checks.  A capacity above DAL_SORT_CAP_PAYLOAD takes the exact
 * level 1 whatever level1_passes (0..5) says.  Workspace:
 * dal_dw_step_workspace_bytes.
 * dal_dw_step_multiclass_form is pure host code: the branch the call takes for
 * a shape -- 0 exact level 1; 1 fast level 1, group-minimum pass; 2 fast,
 * folded by the score kernel with plain stores (one tile per group); 3 fast,
 * folded with atomic maxima (several tiles per group) -- or the negative status
 * the entry's shape checks return.  blocked: non-zero when the call is given xb
 * (and fprep). */
int dal_dw_step_multiclass(const float* x, const float* xb, const void* fprep, int64_t n, int64_t d, int64_t ldx,
                           const int32_t* inner, const uint8_t* leaf, int32_t n_trees, int32_t depth,
                           int32_t n_classes, const double* lut, const int64_t* density_fixed, double density_err,
                           const uint8_t* row_flags, double beta, int64_t idx_base, const double* norm64,
                           const double* colsum, int64_t k, int64_t cap, int32_t level1_passes, uint32_t step_flags,
                           void* ws, size_t ws_bytes, uint8_t* counts, uint8_t* pred, double* entropy,
                           int32_t* row_index, double* scores, uint64_t* keys_lo, uint64_t* keys_hi,
                           int64_t* out_idx, double* out_scores, uint64_t* out_keys, int32_t* dev_status,
                           dal_event_t colsum_ready, dal_stream_t stream);
int dal_dw_step_multiclass_form(int64_t n, int64_t d, int32_t n_trees, int32_t depth, int32_t n_classes, int64_t k,
                                int64_t cap, int32_t level1_passes, int blocked);

/* ---- one density-weighted iteration over a soft-vote forest in one call ---
 * A new symbol only: dal_abi_version() stays 10 (absent from older
 * libraries).  dal_dw_step_soft is equivalent to dal_forest_score_soft_dw(x,
 * ..., density_fixed, DAL_DENSITY_FIXED, density_err, row_flags, beta, sums,
 * pred, entropy, row_index, scores, keys_lo, keys_hi) followed by
 * dal_dw_select(keys_lo, keys_hi, row_index, row_flags, n, k, idx_base,
 * entropy, beta, x, d, x_stride, norm64, colsum, cap, level1_passes, ...) --
 * same outputs, same bits.  The soft kernel does not fold group minima: the
 * step takes the exact level 1 (level1_passes == 0, or a capacity above
 * DAL_SORT_CAP_PAYLOAD whatever level1_passes says), or with the fast level 1
 * one group-minimum pass after the score kernel and then ONE launch that
 * derives tau, appends the candidates with their canonical scores and sorts
 * them.  step_flags: DAL_STEP_RESET_STATUS and DAL_STEP_WS_CLEAN as for
 * dal_dw_step; any other bit is DAL_ERR_ARG.  sums and pred are nullable;
 * every other buffer is required (DAL_ERR_ARG), then the score entry's
 * DAL_ERR_SHAPE and DAL_ERR_UNSUPPORTED checks; n == 0 returns DAL_OK before
 * the selection's checks.  Workspace: dal_dw_step_workspace_bytes. */
int dal_dw_step_soft(const float* x, int64_t n, int64_t d, int64_t x_stride, const int32_t* inner,
                     const int32_t* leaf_id, const uint32_t* leaf_q, int64_t n_leaves, int32_t n_trees,
                     int32_t depth, int32_t n_classes, const int64_t* density_fixed, double density_err,
                     const uint8_t* row_flags, double beta, int64_t idx_base, const double* norm64,
                     const double* colsum, int64_t k, int64_t cap, int32_t level1_passes, uint32_t step_flags,
                     void* ws, size_t ws_bytes, uint64_t* sums, uint8_t* pred, double* entropy, int32_t* row_index,
                     double* scores, uint64_t* keys_lo, uint64_t* keys_hi, int64_t* out_idx, double* out_scores,
                     uint64_t* out_keys, int32_t* dev_status, dal_event_t colsum_ready, dal_stream_t stream);

/* ---- warm-step plan: a replayed dal_dw_step with a one-call host side -----
 * dal_dw_plan_create captures dal_dw_step (DAL_STEP_RESET_STATUS |
 * DAL_STEP_WS_CLEAN, no colsum event) over the given caller-owned buffers as a
 * hipGraph (the workspace is zeroed once, synchronously on ``stream``).
 * ``flags`` is the step's row-flag scratch: runs with the exact level 1
 * (level1_passes = 0) rebuild it from ``base_flags`` (the pool's EXCLUDED
 * bits) and the unlabeled list; with the fast level 1 the re-rank derives its
 * candidates' flags from the step's row stamps and ``flags`` is not written
 * (ABI v7); the
 * selection lands in out_pair[0..k) (indices) and out_pair[k..2k) (fp64
 * score bits).  dal_dw_plan_run(plan, unl, n_unl, out_idx, out_scores,
 * status, stream): flags <- base_flags, mark unl as DAL_ROW_CANDIDATE, replay
 * (the graph's last kernel also writes the selection to out_idx / out_scores
 * -- nullable, k each -- and the final status word to host-mapped memory),
 * wait for that word (a bounded spin, then a stream sync) and return the
 * status in *status -- the
 * density_weighting.py:133-176 iteration in one call.  Buffers must outlive
 * the plan; dal_dw_plan_destroy frees it.  xb (ABI v9) and fprep (ABI v10;
 * both nullable): as dal_dw_step's -- the plan reads fprep at its captured
 * address on every replay, so a new forest is re-prepared into the same
 * buffer before the next run.  A null x, base_flags, flags, out_pair, ws or
 * plan is DAL_ERR_ARG and n < 1, k < 1, d < 1 or ldx < d DAL_ERR_SHAPE, both
 * before the workspace is touched or a capture begun (*plan is then NULL);
 * the step's other checks are made while it is captured. */
typedef struct dal_dw_plan dal_dw_plan_t;
int dal_dw_plan_create(const float* x, const float* xb, const void* fprep, int64_t n, int64_t d, int64_t ldx,
                       const int32_t* inner,
                       const uint8_t* leaf, int32_t n_trees, int32_t depth, const double* lut,
                       const int64_t* density_fixed, double density_err, const uint8_t* base_flags,
                       uint8_t* flags, double beta, int64_t idx_base, const double* norm64,
                       const double* colsum, int64_t k, int64_t cap, int32_t level1_passes, void* ws,
                       size_t ws_bytes, int32_t* votes, double* scores, uint64_t* keys_lo, uint64_t* keys_hi,
                       int64_t* out_pair, uint64_t* out_keys, int32_t* dev_status, dal_stream_t stream,
                       dal_dw_plan_t** plan);
/* The C-class plan: dal_dw_step_multiclass captured the same way (the same
 * mark kernel, stamps, host-mapped slot and status word).  dal_dw_plan_create's
 * arguments with n_classes after depth and counts, pred (both nullable),
 * entropy, row_index in the place of votes; lut is multiclass_lut("entropy", T).
 * dal_dw_plan_run, dal_dw_plan_launch and dal_dw_plan_destroy serve it
 * unchanged.  A new symbol: dal_abi_version() stays 10. */
int dal_dw_plan_create_multiclass(const float* x, const float* xb, const void* fprep, int64_t n, int64_t d,
                                  int64_t ldx, const int32_t* inner, const uint8_t* leaf, int32_t n_trees,
                                  int32_t depth, int32_t n_classes, const double* lut, const int64_t* density_fixed,
                                  double density_err, const uint8_t* base_flags, uint8_t* flags, double beta,
                                  int64_t idx_base, const double* norm64, const double* colsum, int64_t k,
                                  int64_t cap, int32_t level1_passes, void* ws, size_t ws_bytes, uint8_t* counts,
                                  uint8_t* pred, double* entropy, int32_t* row_index, double* scores,
                                  uint64_t* keys_lo, uint64_t* keys_hi, int64_t* out_pair, uint64_t* out_keys,
                                  int32_t* dev_status, dal_stream_t stream, dal_dw_plan_t** plan);
int dal_dw_plan_run(dal_dw_plan_t* plan, const int64_t* unl, int64_t n_unl, int64_t* out_idx,
                    double* out_scores, int32_t* status, dal_stream_t stream);
/* The plan's replay WITHOUT the host wait (ABI v5): refreshes the row marks,
 * launches the graph on ``stream`` and returns.  The outputs stay in the
 * buffers given at creation (out_keys, out_pair = selected indices | score
 * bits, dev_status) -- e.g. one packed row [keys k | indices k | score bits
 * k | status] that a multi-GPU caller all-gathers and merges stream-ordered,
 * reading the status once after the merge. */
int dal_dw_plan_launch(dal_dw_plan_t* plan, const int64_t* unl, int64_t n_unl, dal_stream_t stream);
void dal_dw_plan_destroy(dal_dw_plan_t* plan);

/* ---- (a12, config 5) max-cosine to a labeled set -----------------------
 * Restates similarity.py:26-43 (columnSimilarities of the normalised pool) as
 * m_i = max_{l in L} cos(x_i, x_l) over a bf16 pool (row-major [n][d],
 * d in {64,128,256}) and a bf16 labeled table [m_pad][d] whose rows beyond the
 * real m carry inv_lab = NaN (ignored).  bf16 MFMA (v_mfma_f32_32x32x16_bf16),
 * fp32 accumulate, row-max epilogue; the n x m matrix is never stored.
 * m_pad % dal_maxcos_label_rows_granule(d) == 0, m_pad <= 4096.  inv_pool
 * (nullable): per-row 1/||x_i||; NULL computes it in-kernel (the diagonal of
 * the register-resident row fragments' own Gram, fp32 sums of exact products).
 * |m_gpu - m_canonical| <= dal_maxcos_error_bound(d) (Cauchy-Schwarz). */
int64_t dal_maxcos_label_rows_granule(int64_t d);
double dal_maxcos_error_bound(int64_t d);
int dal_inv_norms_bf16(const uint16_t* x, int64_t n, int64_t n_pad, int64_t d, int64_t ld,
                       float* inv, int32_t* dev_status, dal_stream_t stream);
/* Canonical fp64 unit rows (sequential fp64 norm, then divide) of n bf16
 * rows: u[i * d + f] (feature_major = 0) or u[f * n + i] (feature_major = 1). */
int dal_canon_unit_rows_bf16(const uint16_t* x, int64_t n, int64_t d, int64_t ld, int feature_major,
                             double* u, dal_stream_t stream);
/* out_arg (nullable): the arg-max l (position in the labeled table, first l
 * among equal values) of every row.  A row whose two largest fp32 cosines are
 * within 2 x dal_maxcos_error_bound(d) of each other cannot be ordered from
 * the fp32 values: it gets -1 - l, and dal_maxcos_argmax_resolve replaces
 * every such entry by the canonical fp64 arg-max (similarity.py:34-38,
 * columnSimilarities' exact cosines; ties -> first l).  Every other entry is
 * already the canonical arg-max. */
int dal_max_cosine(const uint16_t* pool, int64_t n, int64_t d, const uint16_t* lab, int64_t m_pad,
                   const float* inv_lab, const float* inv_pool, float* out_max, int32_t* out_arg,
                   int32_t* dev_status, dal_stream_t stream);
/* Max-cosine WITHOUT the arg-max on a folded labeled operand (ABI v7; the
 * diversity selection's values): lab_unit = dal_unit_rows_f16's fp16 table
 * 2^15 x_l / ||x_l|| [m_pad][d] (no per-column scaling left in the kernel:
 * the epilogue is a bare running max).  Each pool row is rescaled by a power
 * of two and converted to fp16 in registers; v_mfma_f32_16x16x32_f16.
 * |m_gpu - m_canonical| <= dal_maxcos_unit_error_bound(d) (~2^-11: the fp16
 * rounding of the unit rows; the selection stays exact through the fp64
 * re-rank).  Rows whose largest |x_if| is zero or a bf16 subnormal flag
 * DAL_FLAG_ZERO_NORM, as in dal_max_cosine. */
int dal_unit_rows_f16(const uint16_t* x, int64_t m, int64_t m_pad, int64_t d, int64_t ld, uint16_t* out,
                      int32_t* dev_status, dal_stream_t stream);
double dal_maxcos_unit_error_bound(int64_t d);
int dal_max_cosine_unit(const uint16_t* pool, int64_t n, int64_t d, const uint16_t* lab_unit, int64_t m_pad,
                        float* out_max, int32_t* dev_status, dal_stream_t stream);
/* Canonical fp64 arg-max (oracle max_cosine_canonical: sequential norm and
 * dot products, no FMA, first l on ties) of every row with out_arg < 0;
 * ulab = canonical fp64 unit rows of the m labeled rows, feature-major [d][m]
 * (dal_canon_unit_rows_bf16 with feature_major = 1); d <= 256. */
int dal_maxcos_argmax_resolve(const uint16_t* pool, int64_t n, int64_t d, int64_t ld, const double* ulab,
                              int64_t m, int32_t* out_arg, dal_stream_t stream);
/* Interval keys [v - err, v + err] of fp32 values (pessimistic -> keys_lo). */
int dal_interval_keys_f32(const float* values, int64_t n, double err, const uint8_t* row_flags,
                          int order, uint64_t* keys_lo, uint64_t* keys_hi, dal_stream_t stream);
/* Diversity selection: the k rows with the smallest canonical fp64 max-cosine
 * (ties -> lower index), from interval keys of dal_max_cosine's output;
 * ulab = canonical fp64 unit rows of the m labeled rows, feature-major
 * [d][m] (dal_canon_unit_rows_bf16 with feature_major = 1); d <= 256.  Same candidate/re-rank contract
 * as dal_dw_select, including level1_passes (0 = exact radix level 1; 1-5 =
 * the fast group-minimum level 1, DAL_FLAG_SAMPLE_MISS when its candidates
 * overflow cap <= 4096). */
size_t dal_maxcos_select_workspace_bytes(int64_t n, int64_t k, int64_t cap);
int dal_maxcos_select(const uint64_t* keys_lo, const uint64_t* keys_hi, int64_t n, int64_t k,
                      int64_t idx_base, const uint16_t* pool, int64_t d, int64_t ld,
                      const double* ulab, int64_t m, int64_t cap, int32_t level1_passes, void* ws,
                      size_t ws_bytes,
                      int64_t* out_idx, double* out_scores, uint64_t* out_keys,
                      int32_t* dev_status, dal_stream_t stream);

/* ---- multi-GPU merge ----------------------------------------------------
 * Sort n (key, idx) pairs (e.g. the all-gathered per-GPU top-k lists) by
 * (key, idx) and keep the first k.  n <= DAL_SORT_CAP.  ``payload`` (nullable)
 * is permuted alongside (then n <= DAL_SORT_CAP_PAYLOAD). */
int dal_sort_pairs(const uint64_t* keys, const int64_t* idx, const double* payload, int64_t n,
                   int64_t k, uint64_t* out_keys, int64_t* out_idx, double* out_payload,
                   dal_stream_t stream);

/* dal_topk_merge: the same merge read straight from one all-gather's output.
 * packed [n_ranks][width] int64 rows = a rank's k keys | k global indices |
 * k fp64 score bit patterns (| its status word at 3k when status_or is
 * given).  Writes the k best by (key, rank-major position) -- ties resolve
 * by global row index -- to out_idx / out_scores, and the OR of the status
 * words to *status_or (nullable), the winners' keys to out_keys (nullable;
 * DAL_KEY_NONE marks padding that won only because fewer than k candidates
 * exist).  n_ranks * k <= DAL_SORT_CAP.  One launch and no workspace (ws may
 * be NULL; dal_topk_merge_workspace_bytes returns 0) when n_ranks * k <=
 * DAL_SORT_CAP_PAYLOAD and n_ranks <= 32: the rows are read in place by the
 * one-block sort, ordered by (key, global index) -- the same order, as ranks
 * hold ascending row ranges; otherwise three launches (unpack, sort, gather).
 * Replaces the sortBy(...).take(k) of density_weighting.py:168,172 across
 * shards (the Spark range-partition sort over all executors). */
size_t dal_topk_merge_workspace_bytes(int64_t n_ranks, int64_t k);
int dal_topk_merge(const int64_t* packed, int64_t n_ranks, int64_t width, int64_t k, void* ws, size_t ws_bytes,
                   int64_t* out_idx, double* out_scores, uint64_t* out_keys, int32_t* status_or,
                   dal_stream_t stream);

/* ---- pool ingest (host-side parser) -------------------------------------
 * Replaces uncertainty_sampling.py:37-42 / density_weighting.py:45-53,59-65
 * (sc.textFile -> split -> LabeledPoint(0 if int(_[-1]) == -1 else 1,
 * np.array(_[:-1]).astype(float)), take(n_samples)).  HOST pointers (the one
 * exception to the device-pointer convention): ``text`` is a byte range of
 * whitespace-separated rows, label last; blank lines are skipped.
 * dal_text_shape: rows (at most max_rows if >= 0) and fields per row.
 * dal_parse_labeled_text: x [rows][cols-1] fp32 = (float)strtod(field) (the
 * bits of np.float64 parsing narrowed to fp32), labels [rows] (label_map 0:
 * -1 -> 0, else 1; 1: as is); x may be pinned memory handed straight to an
 * async H2D copy.  DAL_ERR_SHAPE: ragged rows; DAL_ERR_ARG: a bad field. */
int dal_text_shape(const char* text, size_t len, int64_t max_rows, int64_t* rows, int64_t* cols);
int dal_parse_labeled_text(const char* text, size_t len, int64_t rows, int64_t cols, int label_map, float* x,
                           int64_t* labels, int n_threads);

/* ---- GPU random-forest training ---------------------
 * Replaces RandomForest.trainClassifier(train, numClasses=2,
 * categoricalFeaturesInfo={}, numTrees=T, featureSubsetStrategy="auto",
 * impurity='gini', maxDepth=4, maxBins=32) (uncertainty_sampling.py:71-76,
 * density_weighting.py:119-124; Spark 2.1 MLlib, continuous features, binary
 * labels).  The training rows x [n][ldx] fp32 are the labeled set.
 *
 * dal_rf_find_splits: findSplitsForContinuousFeature per feature over the
 * sample rows (sample_rows nullable = rows 0..n_sample-1; n_sample <=
 * DAL_RF_MAX_SPLIT_SAMPLE): thresholds [d][DAL_RF_MAX_SPLITS] fp32 (ascending),
 * n_splits [d].  num_splits = min(maxBins, n) - 1.  A feature that would emit
 * more than num_splits + 1 thresholds sets DAL_FLAG_RF_SPLITS in *dev_status.
 *
 * dal_rf_train: grows T trees level by level on the given bagging weights
 * [T][n] (integer Poisson counts; 0 = row not drawn) and per-node feature
 * subsets [T][2^max_depth - 1][m] (heap order, evaluation order; MLlib draws
 * both from JVM RNGs, so they are inputs).  Gini gain in fp64 in MLlib's
 * operation order, first maximum over subset order then split index; a node
 * is a leaf when gain <= 0 (or no valid split) or at max_depth; a child is
 * created as a leaf when pure.  Output in dal_forest_score's heap layout:
 * out_inner [T][2^D - 1][2] = (feature, fp32 threshold bits), (0, +inf) below
 * a leaf; out_leaf [T][2^D] = class (first maximum of the weighted counts),
 * a shallow leaf's class repeated over its subtree.  ws: 256-B aligned,
 * dal_rf_train_workspace_bytes(...) bytes: what
 * dal_rf_train_multiclass_workspace_bytes returns at n_classes = 2 (the binary
 * fit runs the C-class level kernels at C = 2, whose split step keeps 64 B of
 * workspace per split node; a level's span, dal_rf_train_level_span, has the
 * C-class interior [class][bin] at C = 2). */
int dal_rf_find_splits(const float* x, int64_t n, int64_t d, int64_t ldx, const int64_t* sample_rows,
                       int64_t n_sample, int32_t num_splits, float* thresholds, int32_t* n_splits,
                       int32_t* dev_status, dal_stream_t stream);
size_t dal_rf_train_workspace_bytes(int64_t n, int64_t d, int32_t n_trees, int32_t max_depth, int32_t m,
                                    int32_t num_splits);
int dal_rf_train(const float* x, int64_t n, int64_t d, int64_t ldx, const uint8_t* labels,
                 const float* thresholds, const int32_t* n_splits, int32_t num_splits, const int32_t* weights,
                 const int32_t* feature_subsets, int32_t m, int32_t n_trees, int32_t max_depth,
                 int32_t min_instances, double min_info_gain, int32_t* out_inner, uint8_t* out_leaf, void* ws,
                 size_t ws_bytes, dal_stream_t stream);

/* ---- GPU random-forest training, C classes --------------------------------
 * RandomForest.trainClassifier(train, numClasses=C, ...) of the same call
 * sites: dal_rf_train with C classes wherever two appear.  New symbols only:
 * dal_abi_version() stays 10 (absent from older libraries).
 * labels [n] are class ids < n_classes, 2 <= n_classes <= DAL_MC_MAX_CLASSES
 * (a larger byte counts as class n_classes - 1: validate before the call).
 * thresholds / n_splits come from dal_rf_find_splits, which does not depend
 * on the labels.  Gini over the C weighted counts in fp64 in MLlib's order:
 * total = sum of the counts, imp = 1, imp -= (c/total)^2 per class in class
 * order (0 when total == 0), gain = parent - (lc/tc) imp_l - (rc/tc) imp_r;
 * first maximum over subset order then split index; leaf rules as
 * dal_rf_train.  Output in dal_forest_score_multiclass's heap layout:
 * out_inner as dal_rf_train, out_leaf [T][2^D] = class id, the first index of
 * the largest weighted count.  At n_classes == 2 the output equals
 * dal_rf_train's byte for byte.  Callers that score the forest keep
 * n_trees <= DAL_MC_MAX_TREES; the trainer itself does not need it.
 * Limits, checked before any HIP call (DAL_ERR_UNSUPPORTED): max_depth <=
 * DAL_RF_MAX_DEPTH, n_classes <= DAL_MC_MAX_CLASSES, and one node's
 * (slot, class, bin) histogram in LDS: m * (num_splits + 2) * n_classes * 4 <=
 * DAL_RF_SPLIT_LDS_BYTES (784 features, m = 28, maxBins 32, 32 classes:
 * 118,272 bytes).  ws: 256-B aligned,
 * dal_rf_train_multiclass_workspace_bytes(...) bytes (0 for bad arguments). */
size_t dal_rf_train_multiclass_workspace_bytes(int64_t n, int64_t d, int32_t n_trees, int32_t max_depth,
                                               int32_t m, int32_t num_splits, int32_t n_classes);
int dal_rf_train_multiclass(const float* x, int64_t n, int64_t d, int64_t ldx, const uint8_t* labels,
                            const float* thresholds, const int32_t* n_splits, int32_t num_splits,
                            const int32_t* weights, const int32_t* feature_subsets, int32_t m, int32_t n_trees,
                            int32_t max_depth, int32_t min_instances, double min_info_gain, int32_t n_classes,
                            int32_t* out_inner, uint8_t* out_leaf, void* ws, size_t ws_bytes,
                            dal_stream_t stream);

/* ---- regression forests: RandomForestModel.predict of a regressor ---------
 * lal_direct_mllib_implementation/classes/active_learner.py:319 (the LAL
 * model, RandomForest.trainRegressor(numTrees=2000) at :363) and MLlib's
 * trees.map(predict).sum / numTrees.  New symbols only: dal_abi_version()
 * stays 10 (absent from older libraries; probe with
 * dal_forest_regress_chunk_trees).  The forest is a complete heap of depth
 * ``depth`` <= DAL_REG_MAX_DEPTH per tree (dal.forest.RegressionForest):
 *   inner_feature[t][h] int32, inner_threshold[t][h] fp64 (the model's value,
 *   NOT rounded), h < 2^depth - 1;  leaf[t][l] fp64, l < 2^depth;
 *   row[feature] <= threshold -> child 2h+1, else 2h+2 (an fp64 compare: a NaN
 *   feature goes right); a shallow leaf's subtree is padded with (0, +inf)
 *   splits and carries its value.
 * x: n rows of d features, row stride ldx elements, fp32 (DAL_X_F32, compared
 * as (double)x <= threshold) or fp64 (DAL_X_F64).
 *   out[i] = (((0.0 + leaf_0(x_i)) + leaf_1(x_i)) + ... + leaf_{T-1}(x_i)) / (double)T
 * sequential fp64 adds in tree order, one division: bit for bit the Python
 * float loop, for every n, d and n_trees.  The kernel streams the forest
 * through LDS dal_forest_regress_chunk_trees(depth) trees at a time (0 for a
 * depth outside [1, DAL_REG_MAX_DEPTH]; non-increasing in depth); a row is
 * summed by one lane from the first tree to the last.
 * n == 0 returns DAL_OK and launches nothing.  Before any launch: a null
 * pointer or an x_dtype other than the two is DAL_ERR_ARG, depth outside
 * [1, DAL_REG_MAX_DEPTH] DAL_ERR_UNSUPPORTED, n_trees < 1, n < 0, d < 1 or
 * ldx < d DAL_ERR_SHAPE.  A feature outside [0, d) is the caller's error (the
 * forest is device data; RegressionForest.check_features checks it before
 * upload): the kernel clamps it into [0, d - 1]. */
#define DAL_REG_MAX_DEPTH 10
#define DAL_X_F32 0
#define DAL_X_F64 1
int dal_forest_regress_chunk_trees(int32_t depth);
int dal_forest_regress(const void* x, int x_dtype, int64_t n, int64_t d, int64_t ldx,
                       const int32_t* inner_feature, const double* inner_threshold, const double* leaf,
                       int32_t n_trees, int32_t depth, double* out, dal_stream_t stream);

/* ---- GPU training of regression forests: exact variance histograms --------
 * RandomForest.trainRegressor(data, categoricalFeaturesInfo={}, numTrees=T,
 * featureSubsetStrategy="auto", impurity="variance", maxDepth=4, maxBins=32)
 * (lal_direct_mllib_implementation/classes/active_learner.py:354-365; Spark 2.1
 * MLlib, continuous features).  New symbols only: dal_abi_version() stays 10
 * (absent from older libraries).
 *
 * As in dal_rf_train: thresholds are findSplitsForContinuousFeature, bins are
 * #{thresholds < x}, split k sends bin <= k left; integer bagging weights
 * [T][n] and per-node feature subsets [T][2^D - 1][m] are inputs; growth is
 * level-wise; the best split is the first maximum over subset order then split
 * index; a node is a leaf when gain <= 0 (or no valid split) or at max_depth; a
 * child is created as a leaf at max_depth or when its impurity == 0.0; a child
 * with a weighted count < min_instances makes a split invalid, and so does
 * gain < min_info_gain.  For regression "auto" means every feature for one
 * tree and ceil(d / 3) for a forest (the caller sizes m).
 *
 * Statistics of a row set R (the canonical semantics):
 *   count = sum_R w (integer), sum = RN(sum_R w y), sumSq = RN(sum_R w fl(y y)),
 * the sums EXACT and RN one rounding to nearest-even fp64.  Left statistics of
 * split k: the rows with bin <= k; right: the exact node sums minus the exact
 * left sums, rounded once (not a difference of rounded values).
 *   impurity = 0 when count == 0, else (sumSq - (sum sum) / count) / count
 *   gain     = impurity - (lc/tc) imp_l - (rc/tc) imp_r
 *   leaf     = sum / count (0 when count == 0)
 * in fp64 in that operation order, no FMA.  This departs from Spark's bits on
 * purpose: Spark adds fl(fl(w y) y) terms in partition order, so its own sums
 * vary in the last places from run to run (and, under cancellation such as
 * labels 1e8 + small, so do its trees); the exact sum is the value every such
 * order approximates, and it makes the fit independent of the order in which
 * atomics arrive.
 *
 * The exact sums (csrc/rf_exact_sum.hpp): the caller describes the labels by
 * (q_y, k_y) and their squares fl(y y) by (q_sq, k_sq): q is the exponent of
 * the lowest set bit over the nonzero values (0 when there are none), and
 * k = max(1, ceil(span / 31)) limbs of 31 bits cover span = (exponent above
 * the highest set bit) - q bits.  k <= DAL_RF_REG_MAX_LIMBS (a span of 248
 * bits; smooth labels need 2 + 3 limbs, labels eleven decades apart 3 + 5),
 * and every tree's weights must sum to less than 2^31 so that no 64-bit word
 * overflows.  A q above a value's lowest set bit, a k too small or a
 * non-finite label is the caller's error (dal.random_forest.train_regressor
 * computes and checks them).
 *
 * dal_rf_find_splits_f64 / dal_rf_bin_rows: dal_rf_find_splits and the binning
 * for rows x [n][ldx] of fp32 (DAL_X_F32) or fp64 (DAL_X_F64): thresholds
 * [d][DAL_RF_MAX_SPLITS] fp64 (the widening of fp32 values is exact; fp64 rows
 * are never rounded), bins [n][d] uint8.  n_sample <= DAL_RF_MAX_SPLIT_SAMPLE
 * for fp32 rows, DAL_RF_MAX_SPLIT_SAMPLE_F64 for fp64 rows (the sort's LDS).
 *
 * dal_rf_train_regressor: bins [n][d], y [n] fp64 -> dal_forest_regress's heap
 * layout: out_feature int32 and out_threshold fp64 [T][2^D - 1], out_leaf fp64
 * [T][2^D]; (0, +inf) below a leaf, a shallow leaf's value repeated over its
 * subtree.  Limits, DAL_ERR_UNSUPPORTED before any HIP call: max_depth <=
 * DAL_RF_MAX_DEPTH, 1 <= k <= DAL_RF_REG_MAX_LIMBS and -1074 <= q <= 1023, and
 * one node's cells in LDS: m * (num_splits + 2) * (1 + k_y + k_sq) * 8 <=
 * DAL_RF_SPLIT_LDS_BYTES.  ws: 256-B aligned,
 * dal_rf_train_regressor_workspace_bytes(...) bytes (0 for bad arguments). */
#define DAL_RF_REG_MAX_LIMBS 8            /* 31-bit limbs per exact sum: label spans up to 248 bits */
#define DAL_RF_MAX_SPLIT_SAMPLE_F64 8192  /* rows one fp64 threshold search sorts in LDS */
int dal_rf_find_splits_f64(const void* x, int x_dtype, int64_t n, int64_t d, int64_t ldx,
                           const int64_t* sample_rows, int64_t n_sample, int32_t num_splits, double* thresholds,
                           int32_t* n_splits, int32_t* dev_status, dal_stream_t stream);
int dal_rf_bin_rows(const void* x, int x_dtype, int64_t n, int64_t d, int64_t ldx, const double* thresholds,
                    const int32_t* n_splits, uint8_t* bins, dal_stream_t stream);
size_t dal_rf_train_regressor_workspace_bytes(int64_t n, int32_t n_trees, int32_t max_depth, int32_t m,
                                              int32_t num_splits, int32_t k_y, int32_t k_sq);
int dal_rf_train_regressor(const uint8_t* bins, int64_t n, int64_t d, const double* y, const double* thresholds,
                           const int32_t* n_splits, int32_t num_splits, const int32_t* weights,
                           const int32_t* feature_subsets, int32_t m, int32_t n_trees, int32_t max_depth,
                           int32_t min_instances, double min_info_gain, int32_t q_y, int32_t k_y, int32_t q_sq,
                           int32_t k_sq, int32_t* out_feature, double* out_threshold, double* out_leaf, void* ws,
                           size_t ws_bytes, dal_stream_t stream);

/* ---- forest training in level steps: the seam of a row-sharded fit ---------
 * MLlib's RandomForest is distributed at this place: every partition fills
 * the (node, feature, bin) aggregates of the current level, they are summed,
 * and the driver picks the splits.  New symbols only: dal_abi_version() stays
 * 10 (absent from older libraries; probe with dal_rf_train_begin).
 *
 * Each trainer is four steps over a caller-owned job descriptor, an opaque
 * blob of DAL_RF_JOB_BYTES bytes (any alignment) that *_begin fills; together
 * with the workspace it is the whole state between calls -- the library keeps
 * none, so jobs are independent and a descriptor may be copied.
 *   *_begin            the argument checks and limits of dal_rf_train /
 *                      dal_rf_train_multiclass / dal_rf_train_regressor over
 *                      the rank's n_local rows, the workspace layout, the
 *                      binning of the local rows (the regressor takes bins, as
 *                      dal_rf_train_regressor does), every tree's root open.
 *                      The descriptor is written once the arguments pass,
 *                      before the first device call.
 *   *_level_stats(l)   zero the level's totals and histogram, then add the
 *                      local rows to them; a row's node of the previous level
 *                      stays in the rank's node [T][n_local].
 *   *_level_split(l)   leaf or best split of every node of the level from the
 *                      totals and the histogram as they then stand in the
 *                      workspace (the same work on every rank); writes the
 *                      split features, split bins and node states.
 *   *_finish           the heap arrays of the outputs given to *_begin.
 * dal_rf_train* are begin, then stats and split for l = 0..max_depth, then
 * finish: the same launches, the same bytes.
 *
 * A sharded fit (the canonical semantics): rank r holds n_local rows of a
 * training set of n_total rows, the weights columns of ITS rows [T][n_local],
 * and the same thresholds, n_splits, num_splits = min(maxBins, n_total) - 1,
 * feature subsets and (regressor) label formats as every other rank.  Between
 * *_level_stats and *_level_split the ranks sum *_level_span element-wise
 * (integers: any order gives the same bytes).  Every rank then holds the
 * forest of the single-device fit of all rows -- for every number of ranks and
 * every assignment of rows to ranks.  n_local == 0 is legal for the steps (x,
 * labels / bins, y and weights may then be null): no row kernel is launched,
 * the span is zeroed, the split runs.  dal_rf_train* keep refusing n < 1.
 * Every tree's weights must sum to less than 2^31 over ALL ranks (int32 class
 * counts and the regressor's 64-bit words alike): the caller's check.
 *
 * *_level_span: ONE contiguous span per level -- ONE collective per level --
 * the totals directly followed by the histogram:
 *   classifiers  DAL_RF_SPAN_I32, T 2^l (C + m hb C) elements,
 *   regressor    DAL_RF_SPAN_I64, T 2^l (W + m hb W) elements,
 * hb = num_splits + 2, W = 1 + k_y + k_sq, C = 2 for dal_rf_train_*; at
 * l == max_depth the totals alone (T 2^l C, T 2^l W).  The address lies in the
 * workspace and is aligned to its element.
 *
 * Before any HIP call: a null pointer, or a descriptor that no *_begin of the
 * same trainer filled, is DAL_ERR_ARG; a level outside [0, max_depth]
 * DAL_ERR_SHAPE; n_local < 0 DAL_ERR_SHAPE; the trainers' limits
 * (DAL_RF_MAX_DEPTH, DAL_MC_MAX_CLASSES, DAL_RF_REG_MAX_LIMBS,
 * DAL_RF_SPLIT_LDS_BYTES) DAL_ERR_UNSUPPORTED, as in dal_rf_train*.  The
 * workspace is dal_rf_train*_workspace_bytes(max(n_local, 1), ...) bytes. */
#define DAL_RF_JOB_BYTES 512
#define DAL_RF_SPAN_I32 0
#define DAL_RF_SPAN_I64 1
int dal_rf_train_begin(void* job, const float* x, int64_t n_local, int64_t d, int64_t ldx, const uint8_t* labels,
                       const float* thresholds, const int32_t* n_splits, int32_t num_splits,
                       const int32_t* weights, const int32_t* feature_subsets, int32_t m, int32_t n_trees,
                       int32_t max_depth, int32_t min_instances, double min_info_gain, int32_t* out_inner,
                       uint8_t* out_leaf, void* ws, size_t ws_bytes, dal_stream_t stream);
int dal_rf_train_level_stats(const void* job, int32_t level, dal_stream_t stream);
int dal_rf_train_level_split(const void* job, int32_t level, dal_stream_t stream);
int dal_rf_train_finish(const void* job, dal_stream_t stream);
int dal_rf_train_level_span(const void* job, int32_t level, void** ptr, int32_t* elem_type, int64_t* count);
int dal_rf_train_multiclass_begin(void* job, const float* x, int64_t n_local, int64_t d, int64_t ldx,
                                  const uint8_t* labels, const float* thresholds, const int32_t* n_splits,
                                  int32_t num_splits, const int32_t* weights, const int32_t* feature_subsets,
                                  int32_t m, int32_t n_trees, int32_t max_depth, int32_t min_instances,
                                  double min_info_gain, int32_t n_classes, int32_t* out_inner, uint8_t* out_leaf,
                                  void* ws, size_t ws_bytes, dal_stream_t stream);
int dal_rf_train_multiclass_level_stats(const void* job, int32_t level, dal_stream_t stream);
int dal_rf_train_multiclass_level_split(const void* job, int32_t level, dal_stream_t stream);
int dal_rf_train_multiclass_finish(const void* job, dal_stream_t stream);
int dal_rf_train_multiclass_level_span(const void* job, int32_t level, void** ptr, int32_t* elem_type,
                                       int64_t* count);
int dal_rf_train_regressor_begin(void* job, const uint8_t* bins, int64_t n_local, int64_t d, const double* y,
                                 const double* thresholds, const int32_t* n_splits, int32_t num_splits,
                                 const int32_t* weights, const int32_t* feature_subsets, int32_t m,
                                 int32_t n_trees, int32_t max_depth, int32_t min_instances, double min_info_gain,
                                 int32_t q_y, int32_t k_y, int32_t q_sq, int32_t k_sq, int32_t* out_feature,
                                 double* out_threshold, double* out_leaf, void* ws, size_t ws_bytes,
                                 dal_stream_t stream);
int dal_rf_train_regressor_level_stats(const void* job, int32_t level, dal_stream_t stream);
int dal_rf_train_regressor_level_split(const void* job, int32_t level, dal_stream_t stream);
int dal_rf_train_regressor_finish(const void* job, dal_stream_t stream);
int dal_rf_train_regressor_level_span(const void* job, int32_t level, void** ptr, int32_t* elem_type,
                                      int64_t* count);

/* ---- LAL query scores from the forest votes --------------------------------
 * active_learner.py:240-343 (ActiveLearnerLAL.selectNext).  The regressor's
 * five features depend on an unlabeled row through its vote count v alone, so
 * its prediction is a table of T + 1 entries (T = n_trees of the classifier,
 * 1 <= T <= DAL_LAL_MAX_TREES, else DAL_ERR_UNSUPPORTED):
 *   votes (dal_forest_score) -> dal_vote_histogram -> dal_lal_rows ->
 *   dal_forest_regress over the T + 1 rows -> dal_votes_rescore -> dal_topk,
 * stream-ordered.  New symbols only: dal_abi_version() stays 10.
 *
 * dal_vote_histogram: hist[v] += #{ i < n : votes[i] == v, row i a
 * DAL_ROW_CANDIDATE } (row_flags NULL: every row counts).  It ACCUMULATES (the
 * caller zeroes hist [T + 1] first), so shards and repeated calls compose;
 * integer atomics, exact in any order.  A vote outside [0, T] is counted
 * nowhere.
 *
 * dal_lal_rows: rows[v] = {f1[v], f2[v], f3, f6, f8} for v = 0..T (the column
 * order of active_learner.py:356) from the (all-reduced) histogram, with
 *   nU = sum_v hist[v] (int64),
 *   f6 = (((0.0 + (double)hist[0] * f2[0]) + (double)hist[1] * f2[1]) + ...
 *         + (double)hist[T] * f2[T]) / (double)nU
 * multiply then add, no FMA, ascending v (:292 in histogram form); nU == 0
 * writes NaN.  f1, f2: fp64 [T + 1] (dal.active_learner.lal_tables).
 *
 * dal_votes_rescore: scores[i] = lut[votes[i]] (fp64 [T + 1]; NaN for a vote
 * outside [0, T]) and keys[i] = dal_forest_score's key of that score for
 * ``order``, DAL_KEY_NONE when the row is not DAL_ROW_CANDIDATE (row_flags
 * NULL: every row is one).  5 bytes read per row: no second forest pass.
 * n == 0 returns DAL_OK and launches nothing; a null pointer or a bad order
 * is DAL_ERR_ARG, n_trees < 1 DAL_ERR_SHAPE (dal_votes_rescore) or
 * DAL_ERR_UNSUPPORTED (the other two), before any launch. */
#define DAL_LAL_MAX_TREES 4095
int dal_vote_histogram(const int32_t* votes, const uint8_t* row_flags, int64_t n, int32_t n_trees,
                       int64_t* hist, dal_stream_t stream);
int dal_lal_rows(const int64_t* hist, const double* f1, const double* f2, int32_t n_trees, double f3, double f8,
                 double* rows, dal_stream_t stream);
int dal_votes_rescore(const int32_t* votes, const uint8_t* row_flags, int64_t n, const double* lut,
                      int32_t n_trees, int order, double* scores, uint64_t* keys, dal_stream_t stream);

/* ---- StandardScaler: exact column moments ----------------------------------
 * lal_direct_mllib_implementation/classes/dataset.py:163-173 (every Dataset*
 * class): MLlib's StandardScaler(withMean=True, withStd=True) over each split.
 * New symbols only: dal_abi_version() stays 10.
 *
 * Canonical semantics.  x: fp32 [n][ldx], d columns, finite.  Per column c,
 * with S1 = sum_i x_ic and S2 = sum_i x_ic^2 as EXACT rationals (an fp32 value
 * is a dyadic rational m 2^e, m < 2^24; its square m^2 2^(2e) has at most 48
 * mantissa bits) and RN64 one rounding to nearest-even fp64:
 *   mean = RN64(S1 / n)
 *   var  = RN64((n S2 - S1^2) / (n (n - 1)))   for n >= 2;  0.0 for n == 1
 *          (MLlib's summarizer returns zero variance when n - 1 is not
 *          positive); the numerator is never negative, so var >= 0
 *   std  = sqrt(var), IEEE fp64: the unbiased sample deviation, as in MLlib
 *   z    = (double(x) - mean) * (1.0 / std)  if std != 0.0, else +0.0
 *          (the dense withMean && withStd branch of MLlib 2.1's
 *          StandardScalerModel.transform), fp64, two roundings, no FMA;
 *          without the mean: double(x) * (1.0 / std); without the deviation:
 *          double(x) - mean
 *   out  = RN32(z) (the double rounding is the definition), or z as fp64.
 * The bits do not depend on the row order, on chunking or on sharding: the
 * sums are integers.  MLlib itself pins no bits (its summarizer merges
 * partition summaries in arrival order); these values are what every such
 * order approximates.
 *
 * The exact sums (csrc/scaler_exact.hpp over csrc/rf_exact_sum.hpp).  Column c
 * is described by low[c], the minimum over its nonzero values of the lowest
 * set bit's exponent, and top[c], the maximum of (the top bit's exponent) + 1
 * (|x| < 2^top); a column of zeros keeps INT32_MAX / INT32_MIN.  The quantum
 * of S1 is 2^q[c] with q[c] = low[c] (0 for a column of zeros), that of S2 is
 * 2^(2 q[c]).  K1 = max_c ceil((top - low) / 31) limbs hold x / 2^q, K2 =
 * max_c ceil(2 (top - low) / 31) limbs hold x^2 / 2^(2q) (each at least 1).
 * Boundary: K2 <= DAL_RF_REG_MAX_LIMBS, i.e. top[c] - low[c] <= 124 bits
 * between a column's lowest and highest set bit.  2^-40 beside 2^20 spans 61
 * bits and passes; an fp32 subnormal (2^-149) beside 1.0 spans 150 and is
 * refused with DAL_ERR_UNSUPPORTED, never answered wrongly.
 *
 * dal_scaler_format: low[c] = min(low[c], ...), top[c] = max(top[c], ...) over
 * the call's rows (int32 atomics; the caller initialises them to INT32_MAX /
 * INT32_MIN, so chunks and shards compose: MIN / MAX are the all-reduce ops),
 * and *dev_status |= DAL_FLAG_NONFINITE when a NaN or an infinity was met.
 *
 * dal_scaler_limbs: host function over HOST arrays low, top [d] -> *k1, *k2,
 * q[d] (nullable) and *bad_column (nullable; -1, or the first column over the
 * boundary, with DAL_ERR_UNSUPPORTED as the status).
 *
 * dal_scaler_accumulate: cells[c][0 .. k1) += limbs of x_ic / 2^q[c] and
 * cells[c][k1 .. k1 + k2) += limbs of x_ic^2 / 2^(2 q[c]) over the call's
 * rows; cells int64 [d][k1 + k2], zeroed by the caller once: calls add, so a
 * pool can be fed in chunks or by shards (SUM is the all-reduce op).  Each
 * word stays below 2^31 * (rows in total), so the total must be <= INT32_MAX
 * rows.  q (device) must not exceed a value's lowest set bit and k1, k2 must
 * cover the spans: both come from the format pass; a non-finite value is the
 * caller's error.  One 64-bit integer atomic per (block, column, word);
 * dal_scaler_rows_per_block(n, d) gives the rows of one block (0 for bad
 * arguments).
 *
 * dal_scaler_transform: out[i][c] (fp32 for DAL_X_F32, fp64 for DAL_X_F64,
 * row stride ldo elements) = the z above with factor[c] = 1.0 / std, or 0.0
 * where std == 0.0 (then +0.0 is written).  mean NULL: no centring; factor
 * NULL: no scaling.
 *
 * Before any launch: a null pointer or a bad out_dtype is DAL_ERR_ARG; n < 0,
 * n > INT32_MAX, d < 1, ldx < d or ldo < d DAL_ERR_SHAPE; k1 or k2 outside
 * [1, DAL_RF_REG_MAX_LIMBS] DAL_ERR_UNSUPPORTED.  n == 0 returns DAL_OK and
 * launches nothing (the cells are untouched). */
int64_t dal_scaler_rows_per_block(int64_t n, int64_t d);
int dal_scaler_limbs(const int32_t* low, const int32_t* top, int64_t d, int32_t* k1, int32_t* k2, int32_t* q,
                     int64_t* bad_column);
int dal_scaler_format(const float* x, int64_t n, int64_t d, int64_t ldx, int32_t* low, int32_t* top,
                      int32_t* dev_status, dal_stream_t stream);
int dal_scaler_accumulate(const float* x, int64_t n, int64_t d, int64_t ldx, const int32_t* q, int32_t k1,
                          int32_t k2, int64_t* cells, dal_stream_t stream);
int dal_scaler_transform(const float* x, int64_t n, int64_t d, int64_t ldx, const double* mean,
                         const double* factor, void* out, int out_dtype, int64_t ldo, dal_stream_t stream);

/* ---- test-set evaluation: joint histogram, exact squared error -------------
 * lal_direct_mllib_implementation/classes/active_learner.py:95-121
 * (ActiveLearner.evaluate: accuracy, TN / TP / FN / FP, auc) and the regressor
 * scripts' testMSE = sum (label - prediction)^2 / count
 * (mllib/mllib_random_forest_regressor.py:48).  New symbols only:
 * dal_abi_version() stays 10; dal_forest_evaluate_cells is the probe (absent
 * from older libraries).
 *
 * dal_forest_evaluate: one fused forest pass over the rows that writes nothing
 * per row.  The forest, x, xb and fprep are dal_forest_score_blocked's and
 * dal_forest_score_multiclass_blocked's (one prepared buffer serves all
 * three); labels: one class id byte per row; a row is counted when row_flags
 * is NULL or carries DAL_ROW_CANDIDATE (as dal_vote_histogram).  hist (int64,
 * dal_forest_evaluate_cells(n_trees, n_classes) words):
 *   n_classes == 2, 1 <= n_trees <= DAL_LAL_MAX_TREES: hist[T + 1][2], cell
 *     [v][y] += rows with v trees whose leaf byte is 1 and label y;
 *   3 <= n_classes <= DAL_MC_MAX_CLASSES, n_trees <= DAL_MC_MAX_TREES:
 *     hist[C][C], cell [y][pred], pred = the smallest class with the most
 *     trees (dal_forest_score_multiclass's pred);
 *   any other (n_trees, n_classes): 0 cells, DAL_ERR_UNSUPPORTED.
 * A row whose label is >= n_classes, or one of whose trees ends in a leaf byte
 * >= n_classes, is counted nowhere (dal.metrics checks both before upload).
 * The call ACCUMULATES (the caller zeroes hist), so shards and repeated calls
 * compose: 32-bit counters per block in LDS, one 64-bit integer atomic per
 * occupied cell per block -- exact in any order, the same words for every
 * grid, row order and sharding.  dal_forest_evaluate_blocked_rows is the rule
 * that picks the kernel: 64 when the score entries' rule holds
 * (dal_forest_blocked_rows; for n_classes > 2 dal_forest_multiclass_blocked_
 * rows) and the block's LDS with the table stays within 96 KiB; the blocked
 * kernel then reads only the features the forest tests and needs fprep.  xb
 * NULL, or a rule value of 0, runs the row-major kernel on x.
 * Before any launch: a null x, inner, leaf, labels or hist is DAL_ERR_ARG;
 * n < 0, n >= 2^32, d < 1, d > 2^30 or ldx < d DAL_ERR_SHAPE; a depth outside
 * [1, DAL_MAX_TREE_DEPTH] or 0 cells DAL_ERR_UNSUPPORTED; then a misaligned xb
 * (16 B), or a null or misaligned fprep where the blocked rule holds,
 * DAL_ERR_ARG.  n == 0 returns DAL_OK and launches nothing.
 *
 * dal_sq_error_format / dal_sq_error_accumulate: with e_i = fl(y_i - pred_i)
 * and s_i = fl(e_i * e_i) (two roundings, no FMA), format takes the atomic min
 * of the lowest set bit's exponent into *low and the atomic max of the
 * exponent above the highest set bit into *top over the nonzero s_i (the
 * caller initialises INT32_MAX / INT32_MIN) and raises DAL_FLAG_NONFINITE in
 * *dev_status for a non-finite s_i; accumulate adds the k limbs
 * (csrc/rf_exact_sum.hpp) of every s_i for the quantum 2^q into cells[k] with
 * 64-bit integer atomics (the caller zeroes; q <= *low and 31 k >= *top - q,
 * as dal.random_forest.exact_sum_format derives them).  The exact sum is
 * 2^q sum_j cells[j] 2^(31 j).  A null pointer is DAL_ERR_ARG, n < 0 or
 * n > INT32_MAX DAL_ERR_SHAPE, k outside [1, DAL_RF_REG_MAX_LIMBS]
 * DAL_ERR_UNSUPPORTED; n == 0 returns DAL_OK and launches nothing. */
int dal_forest_evaluate_cells(int32_t n_trees, int32_t n_classes);
int dal_forest_evaluate_blocked_rows(int64_t d, int32_t n_trees, int32_t depth, int32_t n_classes);
int dal_forest_evaluate(const float* x, const float* xb, const void* fprep, int64_t n, int64_t d, int64_t ldx,
                        const int32_t* inner, const uint8_t* leaf, int32_t n_trees, int32_t depth,
                        int32_t n_classes, const uint8_t* labels, const uint8_t* row_flags, int64_t* hist,
                        dal_stream_t stream);
int dal_sq_error_format(const double* pred, const double* y, int64_t n, int32_t* low, int32_t* top,
                        int32_t* dev_status, dal_stream_t stream);
int dal_sq_error_accumulate(const double* pred, const double* y, int64_t n, int32_t q, int32_t k, int64_t* cells,
                            dal_stream_t stream);

/* ---- greedy k-center batch selection (farthest-first) ----------------------
 * Batch-mode diversity (similarity.py:34-38 reduced to the nearest labeled
 * row) where every pick joins the set the remaining rows are compared with.
 * New symbols only: dal_abi_version() stays 10 (absent from older libraries;
 * probe with dal_kcenter_begin).
 *
 * Canonical semantics.  pool: bf16 [n][ld], d in {64, 128, 256}; cos64 is the
 * cosine of dal_cosine_pairs_resolve / the oracle's max_cosine_canonical (unit
 * rows u = x / ||x|| with the sequential fp64 norm, sum_f u_if * u_jf in
 * ascending f, multiply then add, no FMA).  With L the m labeled rows and C
 * the rows flagged DAL_ROW_CANDIDATE:
 *   m_i(0) = max_{l in L} cos64(i, l)
 *   for t = 1 .. k:  p_t = argmin_{i in C, not picked} m_i(t-1), ties -> the
 *                    lower global index; s_t = m_{p_t}(t-1);
 *                    m_i(t) = max(m_i(t-1), cos64(i, p_t)) for every row.
 * out_idx[t-1] = p_t (global: local row + idx_base), out_score[t-1] = s_t
 * (fp64, non-decreasing in t).  When no candidate is left the step writes
 * index -1 and a NaN score and changes nothing else.
 *
 * The caller's device state, which the steps update in place:
 *   m32       fp32 [n], on entry within dal_kcenter_error_bound(d) of m_i(0)
 *             (dal_max_cosine's out_max); after step t within the same bound
 *             of m_i(t) -- the maximum of values that are each within B of
 *             their canonical counterparts is within B of the canonical
 *             maximum, so the bound does not grow;
 *   row_flags uint8 [n]: DAL_ROW_CANDIDATE marks C; a pick gains
 *             DAL_ROW_PICKED;
 *   inv_norm  fp32 [n] = 1 / ||x_i|| (dal_inv_norms_bf16);
 *   centers   fp64 [d][m + k], feature-major with row stride m + k: the
 *             caller fills the first m columns with the labeled rows'
 *             canonical unit rows (dal_canon_unit_rows_bf16's values); step t
 *             appends column m + t.
 * The job descriptor is a caller-owned blob of DAL_KCENTER_JOB_BYTES bytes
 * (any alignment) that dal_kcenter_begin fills; with the workspace
 * (dal_kcenter_workspace_bytes, 256-B aligned) it is the whole state between
 * calls, as for the forest trainers' level steps.
 *
 *   dal_kcenter_begin    checks every argument on the host, writes the
 *                        descriptor, folds m32 into the per-block minima over
 *                        the live candidates.
 *   dal_kcenter_propose  step t (0-based, 0 <= t < k): the shard's best row
 *                        as a record of DAL_KCENTER_RECORD_BYTES(d) bytes at
 *                        ``record`` (device, 16-B aligned): the ascending key
 *                        of the fp64 value (uint64; DAL_KEY_NONE when the
 *                        shard has no live candidate), the global index
 *                        (int64), the fp64 value, one reserved word (0), the
 *                        row's d bf16 values.  Every live candidate whose m32
 *                        is within 2 B of the shard's fp32 minimum has its
 *                        canonical m_i(t-1) recomputed over the first m + t
 *                        columns of the table -- any number of them, on the
 *                        device.
 *   dal_kcenter_commit   step t: the pick is the minimum (key, index) over
 *                        the n_records records at ``records`` (device, 16-B
 *                        aligned, contiguous; every rank passes the same
 *                        bytes, e.g. all-gathered); writes out_idx[t] and
 *                        out_score[t], marks the row when it is local,
 *                        appends the pick's canonical unit row, and runs the
 *                        update pass over the shard's rows -- the one kernel
 *                        of a step that reads the pool (each row once).
 *   dal_kcenter_select   begin, then k x (propose, commit on the own record),
 *                        all enqueued by one host call.
 * n == 0 is a legal shard (pool, row_flags, m32 and inv_norm may be null): it
 * proposes DAL_KEY_NONE and follows the commits.
 *
 * Before any HIP call: a null pointer, a record that is not 16-B aligned, or a
 * descriptor that no dal_kcenter_begin filled, is DAL_ERR_ARG; d outside
 * {64, 128, 256}, n < 0, n > INT32_MAX, ld < d, ld % 8, m < 1, k < 1,
 * idx_base < 0, a pool, m32 or inv_norm that is not 16-B aligned, a workspace
 * that is short or not 256-B aligned, t outside [0, k) or n_records < 1 are
 * DAL_ERR_SHAPE; m + k > INT32_MAX DAL_ERR_CAPACITY.  A refused begin leaves no
 * job behind.  A zero-norm row raises DAL_FLAG_ZERO_NORM in *dev_status. */
#define DAL_ROW_PICKED 4 /* dal_kcenter_*: the row was picked by an earlier step */
#define DAL_KCENTER_JOB_BYTES 512
#define DAL_KCENTER_RECORD_BYTES(d) (32 + 2 * (size_t)(d))
double dal_kcenter_error_bound(int64_t d);
size_t dal_kcenter_workspace_bytes(int64_t n, int64_t d, int64_t m, int64_t k);
int dal_kcenter_begin(void* job, const uint16_t* pool, int64_t n, int64_t d, int64_t ld, int64_t idx_base,
                      uint8_t* row_flags, float* m32, const float* inv_norm, double* centers, int64_t m, int64_t k,
                      void* ws, size_t ws_bytes, int64_t* out_idx, double* out_score, int32_t* dev_status,
                      dal_stream_t stream);
int dal_kcenter_propose(const void* job, int64_t t, void* record, dal_stream_t stream);
int dal_kcenter_commit(const void* job, int64_t t, const void* records, int64_t n_records, dal_stream_t stream);
int dal_kcenter_select(void* job, const uint16_t* pool, int64_t n, int64_t d, int64_t ld, int64_t idx_base,
                       uint8_t* row_flags, float* m32, const float* inv_norm, double* centers, int64_t m, int64_t k,
                       void* ws, size_t ws_bytes, int64_t* out_idx, double* out_score, int32_t* dev_status,
                       dal_stream_t stream);

/* ---- ranked batch-mode selection (uncertainty x diversity, greedy) ----------
 * The ranked batch-mode rule (Cardoso et al. 2017; modAL's batch uncertainty
 * sampling) as a mode of the k-center job: a per-row weight joins the pick
 * rule.  New symbols only: dal_abi_version() stays 10 (absent from older
 * libraries; probe with dal_kcenter_ranked_attach).
 *
 * Canonical semantics.  The pool, L (m >= 1), C and cos64 are those of
 * dal_kcenter_*.  weight: fp64 [n], finite, in [0, 1] (higher = more wanted);
 * alpha in (0, 1], one number per job.  Every operation is one IEEE fp64
 * operation in this order, no FMA contraction:
 *   b      = 1 - alpha
 *   c_i    = b * w_i
 *   m_i(0) = max_{l in L} cos64(i, l)
 *   for t = 1 .. k:
 *     g_i(t) = alpha * (1 - m_i(t-1)) + c_i
 *     p_t    = argmax_{i in C, not picked} g_i(t), ties -> the lower global
 *              index;  s_t = g_{p_t}(t),  r_t = m_{p_t}(t-1)
 *     m_i(t) = max(m_i(t-1), cos64(i, p_t)) for every row.
 * out_idx[t-1] = p_t, out_score[t-1] = s_t (fp64, non-increasing in t: m only
 * grows), out_sim[t-1] = r_t.  When no candidate is left the step writes
 * index -1 and NaN to both.  alpha = 1 is farthest-first on 1 - m: the picks
 * and similarities of the plain job.
 *
 *   dal_kcenter_ranked_workspace_bytes  the ranked workspace for n rows (c_i,
 *                        the block maxima, the contenders' similarities); 0
 *                        for n < 0 or n > INT32_MAX.
 *   dal_kcenter_ranked_error_bound      B_g = alpha * dal_kcenter_error_bound(d)
 *                        + 2^-48: the bound of the fp32-state score g~_i =
 *                        alpha * (1 - (double)m32_i) + c_i against g_i
 *                        (csrc/kcenter.hip derives it).  Every live candidate
 *                        with g~_i >= max g~ - 2 B_g is re-decided in
 *                        canonical fp64, any number of them.
 *   dal_kcenter_ranked_attach           after dal_kcenter_begin and before the
 *                        first propose of the job: computes c_i into the
 *                        ranked workspace (device, 256-B aligned, kept until
 *                        the last step), refolds the block extremes, and
 *                        switches the descriptor to the ranked mode.
 *                        dal_kcenter_propose / dal_kcenter_commit then serve
 *                        the job with unchanged signatures; the record's
 *                        reserved word carries r (fp64) and its key is that of
 *                        -g, so the minimum (key, index) is still the pick.
 *                        out_sim: fp64 [k], device.
 *   dal_kcenter_run      all k steps of a one-shard job (propose, then commit
 *                        on the job's own record) enqueued by one host call,
 *                        for either mode.
 *
 * Before any HIP call: a null job, workspace or out_sim, a null weight with
 * n > 0, a descriptor that no dal_kcenter_begin filled, or an alpha that is
 * NaN, <= 0 or > 1 is DAL_ERR_ARG; a workspace that is short or not 256-B
 * aligned, or a weight / out_sim that is not 8-B aligned, is DAL_ERR_SHAPE.  A
 * live candidate whose weight is NaN, infinite or outside [0, 1] raises
 * DAL_FLAG_NONFINITE in the job's *dev_status (the selection is then
 * meaningless); the weights of other rows decide nothing. */
size_t dal_kcenter_ranked_workspace_bytes(int64_t n);
double dal_kcenter_ranked_error_bound(int64_t d, double alpha);
int dal_kcenter_ranked_attach(void* job, const double* weight, double alpha, void* ws, size_t ws_bytes,
                              double* out_sim, dal_stream_t stream);
int dal_kcenter_run(const void* job, dal_stream_t stream);

/* ---- standalone similarity kernels --------------------------------------
 * cosine_similarity.py:42-45: every entry of U.U^T (fp32 MFMA), written to
 * out[n_pad][n_pad] (fp32).  similarity.py:38 (columnSimilarities, i<j) is
 * the strict upper triangle of the same matrix. */
int dal_gram_entries(const float* u, int64_t n_pad, int64_t d_pad, int64_t ld, float* out,
                     dal_stream_t stream);

/* ---- thresholded cosine pairs ---------------------------------------------
 * similarity.py:34-38 with a threshold (MLlib's columnSimilarities(threshold),
 * exact here): every pair i < j whose canonical fp64 cosine is >= threshold.
 *
 * dal_cosine_pairs is the filter: a symmetric fp16 MFMA product of the H runs
 * of the split operand (dal_prep_split; rows = the operand of 256-row blocks
 * row_block0 .., cols = the operand whose first row is block col_block0) over
 * the block pairs P <= Q with P in [row_block0, row_block0 + n_row_blocks) and
 * Q in [j_lo, j_hi), global block indices: calls whose ranges tile the blocks
 * cover the upper triangle with no pair twice.  An entry is kept when its
 * filter value (fp32, |value - canonical cosine| <=
 * dal_cosine_pairs_error_bound(d_pad), about 2^-10) is >= threshold - bound
 * (compared against an fp32 threshold rounded down), i < j < n_total, and
 * neither row carries DAL_ROW_EXCLUDED in row_flags (nullable, indexed by
 * global row) -- a superset of the answer.  Candidate c < cap is written as
 * keys[c] = (i << 32) | j, approx[c] = the filter value, in no particular
 * order; *count (zeroed by the caller) is advanced by every candidate, also
 * past cap, where nothing is written and DAL_FLAG_CAND_OVERFLOW is set:
 * *count is then the capacity to retry with.
 *
 * dal_cosine_pairs_resolve writes values[c] = the canonical cosine of
 * candidate c: u = x / norm64 per element in fp64, sum_f u_if * u_jf over the
 * d features in ascending f, multiply then add, no FMA (the oracle's
 * max_cosine_canonical definition; symmetric in (i, j) bit for bit).
 * Membership is values[c] >= threshold in fp64. */
double dal_cosine_pairs_error_bound(int64_t d_pad);
int dal_cosine_pairs(const uint16_t* rows, int64_t row_block0, int64_t n_row_blocks, const uint16_t* cols,
                     int64_t col_block0, int64_t j_lo, int64_t j_hi, int64_t n_total, int64_t d_pad,
                     const uint8_t* row_flags, double threshold, int64_t cap, uint64_t* keys, float* approx,
                     unsigned long long* count, int32_t* dev_status, dal_stream_t stream);
int dal_cosine_pairs_resolve(const float* x, int64_t n, int64_t d, int64_t ldx, const double* norm64,
                             const uint64_t* keys, int64_t n_cand, double* values, dal_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DAL_H */
