// CPU driver of csrc/gram_schedule.hpp at four super blocks per row unit
// (HV = 4, the wide form of gram_csym_kernel) for
// tests/test_gram_schedule_wide.py.  It checks for HV = 4 what
// gram_schedule_driver.cpp and gram_claim_driver.cpp check for HV <= 2: the
// fixed deal through GramCursor, and the kernel's walk through
// GramClaimCursor over sub-slices under three orders of the claims, the fixed
// deal and a counter past the end; the expected set restates the orientation
// rule over unordered pairs.
//   driver sweep     prints "cases N failures M"
//   driver walk NS SROW0 N_SRB J_LO J_HI SKIP_LO SKIP_HI G NC
//                    prints "P J" for every pair of the fixed deal
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "gram_schedule.hpp"

using namespace dal;

namespace {

constexpr int HV = 4;

// {P, Q}, P != Q, belongs to the smaller index when P + Q is even, else to
// the larger; the diagonal to itself.
int owner(int P, int Q) {
  if (P == Q) return P;
  const int lo = P < Q ? P : Q, hi = P < Q ? Q : P;
  return (P + Q) % 2 == 0 ? lo : hi;
}

struct Case {
  int ns, srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi, G, nc, n_slices;
};
enum Order { kTurns, kOneTakesAll, kRandom, kStatic, kCounterPastEnd };

bool expected(const Case& c, int P, int J) {
  return P >= c.srow0 && P < c.srow0 + c.n_srb && P < c.ns && J >= c.j_lo && J < c.j_hi &&
         !(J >= c.skip_lo && J < c.skip_hi) && owner(P, J / 2) == P;
}

int g_failures = 0;
void fail(const Case& c, int order, const char* what, int a, int b) {
  if (++g_failures <= 20)
    printf("FAIL %s (%d, %d): ns %d srow0 %d n_srb %d j [%d, %d) skip [%d, %d) G %d nc %d slices %d order %d\n", what, a,
           b, c.ns, c.srow0, c.n_srb, c.j_lo, c.j_hi, c.skip_lo, c.skip_hi, c.G, c.nc, c.n_slices, order);
}

// rows of the pool a visit may name: the launch's row units reach up to 7
// super blocks past its last one
int p_rows(const Case& c) { return c.ns + 2 * HV + 2; }

void chunks_of(const Case& c, int* chunk_j, int* n_chunks) {
  int64_t cj, nc;
  column_chunks(c.j_hi - c.j_lo, c.nc, &cj, &nc);
  *chunk_j = static_cast<int>(cj);
  *n_chunks = static_cast<int>(nc);
}

// row units: n_ru = 2 * ceil(n_srb / 8); unit ru holds srow0 + 8 * (ru >> 1) + (ru & 1) + 2 h
void check_row_units(const Case& c) {
  int chunk_j, n_chunks;
  chunks_of(c, &chunk_j, &n_chunks);
  const GramSchedule<HV> s(c.srow0, c.n_srb, c.j_lo, c.j_hi, c.skip_lo, c.skip_hi, c.ns, chunk_j, n_chunks, 0, c.G, 0);
  if (s.n_ru != 2 * ((c.n_srb + 7) / 8)) fail(c, -1, "n_ru", s.n_ru, c.n_srb);
  std::vector<int> seen(p_rows(c), 0);
  for (int ru = 0; ru < s.n_ru; ++ru)
    for (int h = 0; h < HV; ++h) {
      const int P = s.rowP(ru, h);
      if (P != c.srow0 + 8 * (ru >> 1) + (ru & 1) + 2 * h || P < 0 || P >= p_rows(c)) {
        fail(c, -1, "rowP", ru, h);
        continue;
      }
      ++seen[P];
    }
  for (int P = c.srow0; P < c.srow0 + c.n_srb; ++P)
    if (seen[P] != 1) fail(c, -1, "super block in no or two row units", P, seen[P]);
}

// the fixed deal (GramCursor), one sub-slice
void walk_static(const Case& c, std::vector<int>& visits, bool print) {
  const int nj2 = 2 * c.ns;
  visits.assign(static_cast<size_t>(p_rows(c)) * nj2, 0);
  int chunk_j, n_chunks;
  chunks_of(c, &chunk_j, &n_chunks);
  for (int g = 0; g < c.G; ++g) {
    const GramSchedule<HV> sched(c.srow0, c.n_srb, c.j_lo, c.j_hi, c.skip_lo, c.skip_hi, c.ns, chunk_j, n_chunks, 0,
                                 c.G, g);
    GramCursor<HV> cur(sched);
    if (!cur.start()) continue;
    while (true) {
      cur.peek();
      int acted = 0;
      for (int h = 0; h < HV; ++h) {
        if (!cur.acts(h)) continue;
        ++acted;
        const int P = sched.rowP(cur.ru, h);
        if (P < 0 || P >= p_rows(c) || cur.J < 0 || cur.J >= nj2) {
          fail(c, kStatic, "visit out of range", P, cur.J);
          continue;
        }
        ++visits[static_cast<size_t>(P) * nj2 + cur.J];
        if (print) printf("%d %d\n", P, cur.J);
      }
      if (!acted) fail(c, kStatic, "pair no part acts on", cur.ru, cur.J);
      if (!cur.has_next) {
        if (!cur.rows_change) fail(c, kStatic, "last pair does not flush", cur.ru, cur.J);
        break;
      }
      const int ru = cur.ru, nru = cur.next_ru, nJ = cur.next_J;
      const bool announced = cur.rows_change;
      const bool changed = cur.advance();
      if (cur.ru != nru || cur.J != nJ) fail(c, kStatic, "advance differs from peek", cur.ru, cur.J);
      if (changed != announced || changed != (cur.ru != ru)) fail(c, kStatic, "rows change", ru, cur.ru);
    }
  }
}

void check_static(const Case& c, std::vector<int>& visits) {
  walk_static(c, visits, false);
  const int nj2 = 2 * c.ns;
  for (int P = 0; P < p_rows(c); ++P)
    for (int J = 0; J < nj2; ++J)
      if (visits[static_cast<size_t>(P) * nj2 + J] != (expected(c, P, J) ? 1 : 0)) fail(c, kStatic, "visits", P, J);
}

// the launch's column chunks tile [j_lo, j_hi) exactly; its units count every sub-slice
void check_launch(const Case& c) {
  for (int min_chunks : {2, 16}) {
    const GramLaunch L = plan_launch<HV>(c.srow0, c.n_srb, c.j_lo, c.j_hi, c.skip_lo, c.skip_hi, c.ns, c.G, 0,
                                         min_chunks, c.n_slices);
    const int nj = c.j_hi - c.j_lo;
    const bool tiles = L.n_chunks >= 1 && L.n_chunks <= nj && L.chunk_j >= 1 &&
                       static_cast<int64_t>(L.n_chunks) * L.chunk_j >= nj &&
                       static_cast<int64_t>(L.n_chunks - 1) * L.chunk_j < nj;
    const int units = 2 * ((c.n_srb + 7) / 8) * L.n_chunks * c.n_slices;
    if (!tiles || L.G < 0 || L.G > c.G || L.units != units) fail(c, -1, "launch", L.n_chunks, L.chunk_j);
  }
  if (GramSchedule<HV>::form_ok(1)) fail(c, -1, "contiguous form accepted", HV, 1);
}

// One launch: the counter the blocks share (the claim is G + its value before
// the add), and what the blocks visited.
struct Launch {
  unsigned next = 0;
  bool counted = true;  // false: the fixed deal
  int G = 1;
  std::vector<int> visits;  // [sub-slice][P][J]
};

// A block of the launch, one pair per step(): the kernel's pair loop with the
// MFMAs replaced by a count and rowacc by the unit whose sums it holds.
struct Block {
  const Case& c;
  Launch& L;
  int order;
  GramSchedule<HV> sched;
  GramClaimCursor<HV> cur;
  bool done = false, started = false;
  int claim_lds = -1;
  int flush_ru = -1;
  int acc_ru = -1, acc_slice = -1;
  int n_units = 0;

  Block(const Case& c_, Launch& L_, int order_, int chunk_j, int n_chunks, int g)
      : c(c_), L(L_), order(order_),
        sched(c_.srow0, c_.n_srb, c_.j_lo, c_.j_hi, c_.skip_lo, c_.skip_hi, c_.ns, chunk_j, n_chunks, 0, c_.G, g),
        cur(sched, c_.n_slices) {}

  void claim_begin() {
    if (L.counted) claim_lds = L.G + static_cast<int>(L.next++);
  }
  int claim_end(int last) { return L.counted ? claim_lds : cur.static_next(last); }
  void claim_take() {
    while (!cur.claimed(claim_end(cur.v_next))) claim_begin();
    if (cur.v_next < cur.total() && cur.c_r < 0) fail(c, order, "empty unit handed over", cur.v_next, 0);
  }
  void flush() {
    if (flush_ru != acc_ru && acc_ru >= 0) fail(c, order, "flush of another unit's rows", flush_ru, acc_ru);
    acc_ru = acc_slice = -1;
    flush_ru = -1;
  }
  void start() {
    started = true;
    if (!cur.claimed(cur.first_unit())) {
      claim_begin();
      claim_take();
    }
    if (!cur.start()) {
      if (cur.v_next < cur.total()) fail(c, order, "walk ends before its claimed unit", cur.v_next, cur.total());
      done = true;
      return;
    }
    ++n_units;
    claim_begin();
  }
  void step() {
    if (!started) return start();
    if (cur.new_unit) claim_take();
    cur.peek();
    if (flush_ru >= 0) flush();
    const int nj2 = 2 * c.ns;
    int acted = 0;
    for (int h = 0; h < HV; ++h) {
      if (!cur.acts(h)) continue;
      ++acted;
      const int P = sched.rowP(cur.ru, h);
      if (P < 0 || P >= p_rows(c) || cur.J < 0 || cur.J >= nj2 || cur.slice < 0 || cur.slice >= c.n_slices) {
        fail(c, order, "visit out of range", P, cur.J);
        continue;
      }
      if (acc_ru >= 0 && (acc_ru != cur.ru || acc_slice != cur.slice))
        fail(c, order, "sums enter rowacc before the flush", acc_ru, cur.ru);
      acc_ru = cur.ru;
      acc_slice = cur.slice;
      ++L.visits[(static_cast<size_t>(cur.slice) * p_rows(c) + P) * nj2 + cur.J];
    }
    if (!acted) fail(c, order, "pair no part acts on", cur.ru, cur.J);
    if (cur.rows_change) flush_ru = cur.ru;
    if (!cur.has_next) {
      if (!cur.rows_change) fail(c, order, "last pair does not flush", cur.ru, cur.J);
      if (cur.v_next < cur.total()) fail(c, order, "walk ends before its claimed unit", cur.v_next, cur.total());
      if (flush_ru >= 0) flush();
      done = true;
      return;
    }
    const int ru = cur.ru, sl = cur.slice, nru = cur.next_ru(), nJ = cur.next_J, nsl = cur.next_slice();
    const bool announced = cur.rows_change, opens = cur.new_unit;
    const bool changed = cur.advance();
    if (cur.ru != nru || cur.J != nJ || cur.slice != nsl) fail(c, order, "advance differs from peek", cur.ru, cur.J);
    if (changed != announced || changed != (cur.ru != ru || cur.slice != sl)) fail(c, order, "rows change", ru, cur.ru);
    if (cur.new_unit != opens) fail(c, order, "new_unit changed by advance", ru, cur.ru);
    if (cur.new_unit) {
      ++n_units;
      claim_begin();
    }
  }
};

unsigned g_rng = 12345u;
unsigned rnd() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng >> 8;
}

void run_claims(const Case& c, int order) {
  const int nj2 = 2 * c.ns;
  Launch L;
  L.G = c.G;
  L.counted = order != kStatic;
  if (order == kCounterPastEnd) L.next = 1u << 20;
  L.visits.assign(static_cast<size_t>(c.n_slices) * p_rows(c) * nj2, 0);
  int chunk_j, n_chunks;
  chunks_of(c, &chunk_j, &n_chunks);
  std::vector<Block> blocks;
  blocks.reserve(c.G);
  for (int g = 0; g < c.G; ++g) blocks.emplace_back(c, L, order, chunk_j, n_chunks, g);
  int live = c.G;
  int64_t steps = 0;
  const int64_t max_steps = int64_t{4} * c.n_slices * p_rows(c) * nj2 + 8 * c.G + 64;
  while (live > 0 && steps <= max_steps) {
    for (int g = 0; g < c.G && live > 0; ++g) {
      Block& b = order == kRandom ? blocks[rnd() % c.G] : blocks[g];
      if (b.done) continue;
      do {
        b.step();
        ++steps;
      } while (order == kOneTakesAll && !b.done && steps <= max_steps);
      if (b.done) --live;
    }
  }
  if (live > 0) return fail(c, order, "walk does not end", live, static_cast<int>(steps));
  if (order == kCounterPastEnd) {
    for (const auto& b : blocks)
      if (b.n_units > 1) fail(c, order, "unit entered from a claim past the end", b.n_units, 0);
    for (int v : L.visits)
      if (v > 1) fail(c, order, "pair visited twice", v, 0);
    return;
  }
  for (int sl = 0; sl < c.n_slices; ++sl)
    for (int P = 0; P < p_rows(c); ++P)
      for (int J = 0; J < nj2; ++J)
        if (L.visits[(static_cast<size_t>(sl) * p_rows(c) + P) * nj2 + J] != (expected(c, P, J) ? 1 : 0))
          fail(c, order, "visits", P, J);
}

// ns_active 1..17 (every n_srb % 8 as the whole pool, with and without a
// padding super block), shard rows from an even and an odd super block, whole
// and half column ranges, no skip range, the shard's own columns and one inside
// the columns, G in {1, 3, 5, 7}, 1..4 requested chunks, 1..3 slices (2..6
// sub-slices)
int sweep() {
  std::vector<int> visits;
  int64_t cases = 0;
  for (int ns = 1; ns <= 17; ++ns)
    for (int srow0 : {0, 1, 2, ns / 2}) {
      if (srow0 >= ns) continue;
      if ((srow0 == 1 || srow0 == 2) && srow0 == ns / 2) continue;  // (listed once)
      for (int n_srb : {ns - srow0 + 1, ns - srow0, (ns - srow0 + 1) / 2, 1}) {
        if (n_srb < 1) continue;
        for (int j_lo = 0; j_lo < 2 * ns; j_lo += 5)
          for (int j_hi : {2 * ns, j_lo + (2 * ns - j_lo + 1) / 2}) {
            if (j_hi <= j_lo) continue;
            const int skips[3][2] = {{0, 0}, {2 * srow0, 2 * (srow0 + n_srb)}, {j_lo + 1, j_lo + 3}};
            for (const auto& sk : skips)
              for (int G : {1, 3, 5, 7}) {
                Case c{ns, srow0, n_srb, j_lo, j_hi, sk[0], sk[1], G, 1, 1};
                check_row_units(c);
                for (int n_slices = 1; n_slices <= 3; ++n_slices) {
                  c.n_slices = 2 * n_slices;  // sub-slices
                  c.nc = 1;
                  check_launch(c);
                  for (int nc = 1; nc <= 4; ++nc) {
                    c.nc = nc;
                    if (n_slices == 1) {
                      check_static(c, visits);
                      ++cases;
                    }
                    for (int order : {kTurns, kOneTakesAll, kRandom, kStatic, kCounterPastEnd}) {
                      run_claims(c, order);
                      ++cases;
                    }
                  }
                }
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
  if (argc == 11 && !strcmp(argv[1], "walk")) {
    int v[9];
    for (int i = 0; i < 9; ++i) v[i] = atoi(argv[2 + i]);
    const Case c{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], 1};
    std::vector<int> visits;
    walk_static(c, visits, true);
    return g_failures ? 1 : 0;
  }
  fprintf(stderr, "usage: %s sweep | walk NS SROW0 N_SRB J_LO J_HI SKIP_LO SKIP_HI G NC\n", argv[0]);
  return 2;
}
