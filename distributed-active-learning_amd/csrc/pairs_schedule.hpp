// The tile schedule of the thresholded cosine pair filter (gram_pairs.hip):
// which block multiplies which 128 x 128 tile of which (256-row block P,
// 256-row block Q) pair.  Integer arithmetic only (one fp64 square root, fixed
// up by integer steps), no HIP header: the kernel and its launcher both use
// this file, and tests/test_pairs_schedule.py walks it on the CPU
// (tests/host/pairs_schedule_driver.cpp).
//
// One call covers row blocks [row_block0, row_block0 + n_row_blocks) against
// column blocks [j_lo, j_hi), global indices, and takes the pairs P <= Q of
// that rectangle: each unordered pair {P, Q} of the pool belongs to exactly one
// (row block, column block) cell, so calls whose row ranges partition the rows
// and whose column ranges partition the columns of each row range cover the
// upper triangle with no pair twice.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define DAL_PAIRS_HD __host__ __device__ __forceinline__
#else
#define DAL_PAIRS_HD inline
#endif

namespace dal {

constexpr int kPairBlock = 256;  // rows of a block P or Q
constexpr int kPairTile = 128;   // rows and columns of one thread block's output tile
constexpr int kPairSubTiles = (kPairBlock / kPairTile) * (kPairBlock / kPairTile);

struct BlockPair {
  int64_t P, Q;
};

struct PairSchedule {
  // Rows below j_lo take every column block of the call (a rectangle, `rect`
  // pairs, `w` per row); rows from j_lo on take the column blocks from their
  // own on (a triangle whose first row p0 has m pairs, the next m - 1, ...).
  int64_t r0, jl, rect_rows, w, p0, tri_rows, m, rect, total;

  DAL_PAIRS_HD PairSchedule(int64_t row_block0, int64_t n_row_blocks, int64_t j_lo, int64_t j_hi) {
    r0 = row_block0;
    jl = j_lo;
    int64_t r1 = row_block0 + n_row_blocks;
    if (r1 > j_hi) r1 = j_hi;  // a row block at or past j_hi takes nothing
    if (r1 < r0) r1 = r0;
    const int64_t re = r1 < j_lo ? r1 : j_lo;  // end of the rectangle's rows
    rect_rows = re > r0 ? re - r0 : 0;
    w = j_hi > j_lo ? j_hi - j_lo : 0;
    p0 = r0 > j_lo ? r0 : j_lo;
    tri_rows = r1 > p0 ? r1 - p0 : 0;
    m = j_hi - p0;
    rect = rect_rows * w;
    total = rect + tri_before(tri_rows);
  }

  // pairs of the triangle's first k rows: m + (m - 1) + ... + (m - k + 1)
  DAL_PAIRS_HD int64_t tri_before(int64_t k) const { return k * (2 * m - k + 1) / 2; }

  // the t-th pair of the call, 0 <= t < total (row-major: P ascending, then Q)
  DAL_PAIRS_HD BlockPair pair(int64_t t) const {
    if (t < rect) return {r0 + t / w, jl + t % w};
    const int64_t u = t - rect;
    // largest k with tri_before(k) <= u: the root of k^2 - (2m + 1) k + 2u = 0,
    // then exact integer steps (the fp64 root may be off by one)
    const double b = static_cast<double>(2 * m + 1);
    int64_t k = static_cast<int64_t>((b - __builtin_sqrt(b * b - 8.0 * static_cast<double>(u))) * 0.5);
    if (k < 0) k = 0;
    if (k > tri_rows - 1) k = tri_rows - 1;
    while (k > 0 && tri_before(k) > u) --k;
    while (k + 1 < tri_rows && tri_before(k + 1) <= u) ++k;
    return {p0 + k, p0 + k + (u - tri_before(k))};
  }

  // Tiles: 4 per pair, tile index = pair * 4 + sub; sub tile (sr, sc) covers
  // rows P * 256 + sr * 128 .. and columns Q * 256 + sc * 128 ...  On the
  // diagonal (P == Q) the sub tile below it (sr > sc) holds only i > j.
  DAL_PAIRS_HD int64_t tiles() const { return total * kPairSubTiles; }
  static DAL_PAIRS_HD int sub_row(int sub) { return sub >> 1; }
  static DAL_PAIRS_HD int sub_col(int sub) { return sub & 1; }
  static DAL_PAIRS_HD bool sub_live(int64_t P, int64_t Q, int sub) { return P != Q || sub_row(sub) <= sub_col(sub); }
};

}  // namespace dal
