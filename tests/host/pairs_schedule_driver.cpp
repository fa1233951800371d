// CPU driver of csrc/pairs_schedule.hpp for tests/test_pairs_schedule.py:
// walks the linear tile index of the thresholded cosine pair filter exactly as
// pairs_filter_kernel's blocks do and compares what it visits with the rule
// restated here as a predicate.
//   driver sweep         block counts 1..40, every split of the rows and of the
//                        columns into two ranges; prints "cases N failures M"
//   driver walk R0 NR J_LO J_HI
//                        prints "P Q live-sub-tiles" for every pair of one call
//   driver large NB      walks every pair of a whole-pool call of NB blocks
//                        (the fp64 root of the index map, fixed up by integer
//                        steps); prints "pairs N failures M"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pairs_schedule.hpp"

using namespace dal;

namespace {

// the rule: a call takes (P, Q) iff P is one of its rows, Q one of its columns, and P <= Q
bool expected(int64_t r0, int64_t nr, int64_t j_lo, int64_t j_hi, int64_t P, int64_t Q) {
  return P >= r0 && P < r0 + nr && Q >= j_lo && Q < j_hi && P <= Q;
}

int g_failures = 0;
void fail(const char* what, int64_t a, int64_t b, int64_t c, int64_t d) {
  if (++g_failures <= 20) printf("FAIL %s %lld %lld %lld %lld\n", what, (long long)a, (long long)b, (long long)c, (long long)d);
}

// adds the call's pairs to seen[P * nb + Q]; checks the call against the rule
void walk_call(int64_t nb, int64_t r0, int64_t nr, int64_t j_lo, int64_t j_hi, std::vector<int>& seen) {
  const PairSchedule s(r0, nr, j_lo, j_hi);
  int64_t want = 0;
  for (int64_t P = 0; P < nb; ++P)
    for (int64_t Q = 0; Q < nb; ++Q) want += expected(r0, nr, j_lo, j_hi, P, Q);
  if (s.total != want) fail("total", r0, nr, j_lo, j_hi);
  if (s.tiles() != s.total * kPairSubTiles) fail("tiles", r0, nr, j_lo, j_hi);
  int64_t lastP = -1, lastQ = -1;
  for (int64_t t = 0; t < s.total; ++t) {
    const BlockPair bp = s.pair(t);
    if (bp.P < 0 || bp.P >= nb || bp.Q < 0 || bp.Q >= nb || !expected(r0, nr, j_lo, j_hi, bp.P, bp.Q)) {
      fail("pair outside the call", t, bp.P, bp.Q, r0);
      continue;
    }
    if (bp.P < lastP || (bp.P == lastP && bp.Q <= lastQ)) fail("order", t, bp.P, bp.Q, r0);
    lastP = bp.P;
    lastQ = bp.Q;
    ++seen[bp.P * nb + bp.Q];
    // live sub tiles: all four off the diagonal; on it, those with an entry i < j
    for (int sub = 0; sub < kPairSubTiles; ++sub) {
      const int sr = PairSchedule::sub_row(sub), sc = PairSchedule::sub_col(sub);
      const int64_t i_min = bp.P * kPairBlock + sr * kPairTile;
      const int64_t j_max = bp.Q * kPairBlock + sc * kPairTile + kPairTile - 1;
      if (PairSchedule::sub_live(bp.P, bp.Q, sub) != (i_min < j_max)) fail("sub tile", bp.P, bp.Q, sub, 0);
    }
  }
}

int sweep() {
  int64_t cases = 0;
  for (int64_t nb = 1; nb <= 40; ++nb) {
    // a: rows [0, a) and [a, nb); b: columns [0, b) and [b, nb) -- a or b at
    // an end leaves one range empty (the single-call case)
    for (int64_t a = 0; a <= nb; ++a)
      for (int64_t b = 0; b <= nb; ++b) {
        std::vector<int> seen(static_cast<size_t>(nb * nb), 0);
        const int64_t rr[2][2] = {{0, a}, {a, nb - a}};
        const int64_t cc[2][2] = {{0, b}, {b, nb}};
        for (int r = 0; r < 2; ++r)
          for (int c = 0; c < 2; ++c) {
            if (rr[r][1] <= 0) continue;  // (the ABI rejects an empty row range)
            walk_call(nb, rr[r][0], rr[r][1], cc[c][0], cc[c][1], seen);
          }
        for (int64_t P = 0; P < nb; ++P)
          for (int64_t Q = 0; Q < nb; ++Q)
            if (seen[P * nb + Q] != (P <= Q ? 1 : 0)) fail("coverage", nb, a * 1000 + b, P, Q);
        ++cases;
      }
    // a row range reaching past the column range, and columns starting inside the rows
    std::vector<int> seen(static_cast<size_t>(nb * nb), 0);
    walk_call(nb, 0, nb + 3, nb / 3, nb - nb / 4, seen);
    ++cases;
  }
  printf("cases %lld failures %d\n", (long long)cases, g_failures);
  return g_failures ? 1 : 0;
}

int large(int64_t nb) {
  const PairSchedule s(0, nb, 0, nb);
  int64_t t = 0;
  for (int64_t P = 0; P < nb; ++P)
    for (int64_t Q = P; Q < nb; ++Q, ++t) {
      const BlockPair bp = s.pair(t);
      if (bp.P != P || bp.Q != Q) fail("large", t, bp.P, bp.Q, P);
    }
  if (t != s.total) fail("large total", t, s.total, 0, 0);
  printf("pairs %lld failures %d\n", (long long)t, g_failures);
  return g_failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc == 3 && !strcmp(argv[1], "large")) return large(atoll(argv[2]));
  if (argc == 6 && !strcmp(argv[1], "walk")) {
    const PairSchedule s(atoll(argv[2]), atoll(argv[3]), atoll(argv[4]), atoll(argv[5]));
    for (int64_t t = 0; t < s.total; ++t) {
      const BlockPair bp = s.pair(t);
      int live = 0;
      for (int sub = 0; sub < kPairSubTiles; ++sub) live += PairSchedule::sub_live(bp.P, bp.Q, sub);
      printf("%lld %lld %d\n", (long long)bp.P, (long long)bp.Q, live);
    }
    return 0;
  }
  fprintf(stderr, "usage: driver sweep | walk R0 NR J_LO J_HI | large NB\n");
  return 2;
}
