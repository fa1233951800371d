// CPU driver of csrc/gram_schedule.hpp for tests/test_gram_schedule.py: walks
// every block of a launch with the header's cursor, exactly as
// gram_csym_kernel's pair loop does, and compares what it visits with the
// orientation rule restated here in its unordered-pair form.
//   driver sweep                    the whole sweep; prints "cases N failures M"
//   driver walk NS SROW0 N_SRB J_LO J_HI SKIP_LO SKIP_HI G CONTIG HV NC
//                                   prints "P J" for every visited pair
//   driver choose G0 HV MIN_CHUNKS NS
//                                   prints "n_chunks chunk_j" of a whole-pool launch
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "gram_schedule.hpp"

using namespace dal;

namespace {

// {P, Q}, P != Q, belongs to the smaller index when P + Q is even, else to
// the larger; the diagonal to itself.
int owner(int P, int Q) {
  if (P == Q) return P;
  const int lo = P < Q ? P : Q, hi = P < Q ? Q : P;
  return (P + Q) % 2 == 0 ? lo : hi;
}

struct Case {
  int ns, srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi, G, contig, nc;
};

bool skipped(const Case& c, int J) { return J >= c.skip_lo && J < c.skip_hi; }
bool expected(const Case& c, int P, int J) {
  return P >= c.srow0 && P < c.srow0 + c.n_srb && P < c.ns && J >= c.j_lo && J < c.j_hi && !skipped(c, J) &&
         owner(P, J / 2) == P;
}

int g_failures = 0;
void fail(const Case& c, int hv, const char* what, int a, int b) {
  if (++g_failures <= 20)
    printf("FAIL %s (%d, %d): ns %d srow0 %d n_srb %d j [%d, %d) skip [%d, %d) G %d contig %d hv %d nc %d\n", what, a, b,
           c.ns, c.srow0, c.n_srb, c.j_lo, c.j_hi, c.skip_lo, c.skip_hi, c.G, c.contig, hv, c.nc);
}

// The kernel's pair loop over every block of the launch: visits[P * nj2 + J]
// counts the (P, J) a half acted on.  Checks the look-ahead against the advance.
template <int HV>
void walk(const Case& c, std::vector<int>& visits, bool print) {
  const int nj2 = 2 * c.ns;
  visits.assign(static_cast<size_t>(c.ns + 2) * nj2, 0);
  int64_t chunk_j = c.j_hi - c.j_lo, n_chunks = 1;
  if (!c.contig) column_chunks(c.j_hi - c.j_lo, c.nc, &chunk_j, &n_chunks);
  if (!GramSchedule<HV>::form_ok(c.contig)) return fail(c, HV, "form", HV, c.contig);
  for (int g = 0; g < c.G; ++g) {
    const GramSchedule<HV> sched(c.srow0, c.n_srb, c.j_lo, c.j_hi, c.skip_lo, c.skip_hi, c.ns,
                                 static_cast<int>(chunk_j), static_cast<int>(n_chunks), c.contig, c.G, g);
    GramCursor<HV> cur(sched);
    if (!cur.start()) continue;
    while (true) {
      cur.peek();
      for (int h = 0; h < HV; ++h) {
        if (!cur.acts(h)) continue;
        const int P = sched.rowP(cur.ru, h);
        if (P < 0 || P > c.ns + 1 || cur.J < 0 || cur.J >= nj2) {
          fail(c, HV, "visit out of range", P, cur.J);
          continue;
        }
        ++visits[static_cast<size_t>(P) * nj2 + cur.J];
        if (print) printf("%d %d\n", P, cur.J);
      }
      if (!cur.has_next) {
        if (!cur.rows_change) fail(c, HV, "last pair does not flush", cur.ru, cur.J);
        break;
      }
      const int ru = cur.ru, nru = cur.next_ru, nJ = cur.next_J;
      const bool announced = cur.rows_change;
      const bool changed = cur.advance();
      if (cur.ru != nru || cur.J != nJ) fail(c, HV, "advance differs from peek", cur.ru, cur.J);
      if (changed != announced || changed != (cur.ru != ru)) fail(c, HV, "rows change", ru, cur.ru);
    }
  }
}

template <int HV>
void check_case(const Case& c, std::vector<int>& visits) {
  walk<HV>(c, visits, false);
  const int nj2 = 2 * c.ns;
  for (int P = 0; P < c.ns + 2; ++P)
    for (int J = 0; J < nj2; ++J)
      if (visits[static_cast<size_t>(P) * nj2 + J] != (expected(c, P, J) ? 1 : 0)) fail(c, HV, "visits", P, J);
}

// (c) pairs_skip against the brute-force count, every P of the pool
void check_pairs_skip(const Case& c) {
  for (int P = 0; P <= c.ns; ++P) {
    int64_t n = 0;
    for (int J = c.j_lo; J < c.j_hi; ++J) n += !skipped(c, J) && owner(P, J / 2) == P;
    if (pairs_skip(P, c.j_lo, c.j_hi, c.skip_lo, c.skip_hi) != n) fail(c, 0, "pairs_skip", P, static_cast<int>(n));
  }
}

// (d) the launch's column chunks tile [j_lo, j_hi) exactly
template <int HV>
void check_launch(const Case& c, int contig) {
  for (int min_chunks : {2, 16}) {
    const GramLaunch L =
        plan_launch<HV>(c.srow0, c.n_srb, c.j_lo, c.j_hi, c.skip_lo, c.skip_hi, c.ns, c.G, contig, min_chunks);
    const int nj = c.j_hi - c.j_lo;
    const bool tiles = L.n_chunks >= 1 && L.n_chunks <= nj && L.chunk_j >= 1 &&
                       static_cast<int64_t>(L.n_chunks) * L.chunk_j >= nj &&
                       static_cast<int64_t>(L.n_chunks - 1) * L.chunk_j < nj;
    if (!tiles || (contig && L.n_chunks != 1) || L.G < 0 || L.G > c.G) fail(c, HV, "launch", L.n_chunks, L.chunk_j);
  }
}

int sweep() {
  std::vector<int> visits;
  int64_t cases = 0;
  for (int ns = 1; ns <= 9; ++ns)
    for (int srow0 = 0; srow0 < ns; ++srow0)
      for (int n_srb = 1; n_srb <= ns - srow0 + 1; ++n_srb)
        for (int j_lo = 0; j_lo < 2 * ns; j_lo += 3)
          for (int j_hi = j_lo + 1; j_hi <= 2 * ns; j_hi += 2) {
            const int skips[3][2] = {{0, 0}, {2 * srow0, 2 * (srow0 + n_srb)}, {j_lo + 1, j_lo + 3}};
            for (const auto& sk : skips) {
              Case c{ns, srow0, n_srb, j_lo, j_hi, sk[0], sk[1], 1, 0, 1};
              check_pairs_skip(c);
              for (int G : {1, 3, 5, 7}) {
                c.G = G;
                c.contig = 1;
                c.nc = 1;
                check_case<1>(c, visits);
                check_launch<1>(c, 1);
                check_launch<1>(c, 0);
                check_launch<2>(c, 0);
                ++cases;
                c.contig = 0;
                for (int nc = 1; nc <= 4; ++nc) {
                  c.nc = nc;
                  check_case<1>(c, visits);
                  check_case<2>(c, visits);
                  cases += 2;
                }
              }
            }
          }
  printf("cases %lld failures %d\n", static_cast<long long>(cases), g_failures);
  return g_failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc == 13 && !strcmp(argv[1], "walk")) {
    int v[11];
    for (int i = 0; i < 11; ++i) v[i] = atoi(argv[2 + i]);
    const Case c{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[10]};
    std::vector<int> visits;
    if (v[9] == 1)
      walk<1>(c, visits, true);
    else
      walk<2>(c, visits, true);
    return g_failures ? 1 : 0;
  }
  if (argc == 6 && !strcmp(argv[1], "choose")) {
    const int64_t G0 = atoll(argv[2]), min_chunks = atoll(argv[4]), ns = atoll(argv[5]);
    const GramLaunch L = atoi(argv[3]) == 1 ? plan_launch<1>(0, ns, 0, 2 * ns, 0, 0, ns, G0, 0, min_chunks)
                                            : plan_launch<2>(0, ns, 0, 2 * ns, 0, 0, ns, G0, 0, min_chunks);
    printf("%d %d\n", L.n_chunks, L.chunk_j);
    return 0;
  }
  fprintf(stderr, "usage: %s sweep | walk ... | choose G0 HV MIN_CHUNKS NS\n", argv[0]);
  return 2;
}
