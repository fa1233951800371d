// CPU driver of GramClaimCursor (csrc/gram_schedule.hpp) for
// tests/test_gram_claim_schedule.py: G simulated blocks walk one launch as
// gram_csym_kernel's pair loop does, taking their units from one shared
// counter, in three orders of the claims -- the blocks step in turn, one
// block runs to its end before the others start (it claims everything), a
// seeded random interleaving -- and with the fixed deal (no counter).
//   driver sweep     prints "cases N failures M"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "gram_schedule.hpp"

using namespace dal;

namespace {

// sb_takes restated over unordered pairs: {P, Q}, P != Q, belongs to the
// smaller index when P + Q is even, else to the larger; the diagonal to itself.
int owner(int P, int Q) {
  if (P == Q) return P;
  const int lo = P < Q ? P : Q, hi = P < Q ? Q : P;
  return (P + Q) % 2 == 0 ? lo : hi;
}

struct Case {
  int ns, srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi, G, contig, nc, n_slices;
};
enum Order { kTurns, kOneTakesAll, kRandom, kStatic, kCounterPastEnd };

bool expected(const Case& c, int P, int J) {
  return P >= c.srow0 && P < c.srow0 + c.n_srb && P < c.ns && J >= c.j_lo && J < c.j_hi &&
         !(J >= c.skip_lo && J < c.skip_hi) && owner(P, J / 2) == P;
}

int g_failures = 0;
void fail(const Case& c, int hv, int order, const char* what, int a, int b) {
  if (++g_failures <= 20)
    printf("FAIL %s (%d, %d): ns %d srow0 %d n_srb %d j [%d, %d) skip [%d, %d) G %d contig %d hv %d nc %d slices %d "
           "order %d\n",
           what, a, b, c.ns, c.srow0, c.n_srb, c.j_lo, c.j_hi, c.skip_lo, c.skip_hi, c.G, c.contig, hv, c.nc,
           c.n_slices, order);
}

// One launch: the counter the blocks share (the kernel's {next} word; the
// claim is G + its value before the add), and what the blocks visited.
struct Launch {
  unsigned next = 0;
  bool counted = true;  // false: the fixed deal
  int G = 1;
  std::vector<int> visits;  // [slice][P][J]
};

// A block of the launch, one pair per step(): the kernel's pair loop with the
// MFMAs replaced by a count and rowacc by the unit whose sums it holds.
template <int HV>
struct Block {
  const Case& c;
  Launch& L;
  int order;
  GramSchedule<HV> sched;
  GramClaimCursor<HV> cur;
  bool done = false, started = false;
  int claim_lds = -1;                 // the value claim_begin left for the block
  int flush_ru = -1;                  // row unit whose sums wait in rowacc
  int acc_ru = -1, acc_slice = -1;    // whose sums rowacc holds (-1: none)
  int n_units = 0;                    // units entered

  Block(const Case& c_, Launch& L_, int order_, int chunk_j, int n_chunks, int g)
      : c(c_), L(L_), order(order_),
        sched(c_.srow0, c_.n_srb, c_.j_lo, c_.j_hi, c_.skip_lo, c_.skip_hi, c_.ns, chunk_j, n_chunks, c_.contig, c_.G,
              g),
        cur(sched, c_.n_slices) {}

  void claim_begin() {
    if (L.counted) claim_lds = L.G + static_cast<int>(L.next++);
  }
  int claim_end(int last) { return L.counted ? claim_lds : cur.static_next(last); }
  void claim_take() {
    while (!cur.claimed(claim_end(cur.v_next))) claim_begin();
    if (cur.v_next < cur.total() && cur.c_r < 0) fail(c, HV, order, "empty unit handed over", cur.v_next, 0);
  }
  void flush() {
    if (flush_ru != acc_ru && acc_ru >= 0) fail(c, HV, order, "flush of another unit's rows", flush_ru, acc_ru);
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
      if (cur.v_next < cur.total()) fail(c, HV, order, "walk ends before its claimed unit", cur.v_next, cur.total());
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
    for (int h = 0; h < HV; ++h) {
      if (!cur.acts(h)) continue;
      const int P = sched.rowP(cur.ru, h);
      if (P < 0 || P > c.ns + 1 || cur.J < 0 || cur.J >= nj2 || cur.slice < 0 || cur.slice >= c.n_slices) {
        fail(c, HV, order, "visit out of range", P, cur.J);
        continue;
      }
      // rowacc holds nothing, or this unit's rows of this slice
      if (acc_ru >= 0 && (acc_ru != cur.ru || acc_slice != cur.slice))
        fail(c, HV, order, "sums enter rowacc before the flush", acc_ru, cur.ru);
      acc_ru = cur.ru;
      acc_slice = cur.slice;
      ++L.visits[(static_cast<size_t>(cur.slice) * (c.ns + 2) + P) * nj2 + cur.J];
    }
    if (cur.rows_change) flush_ru = cur.ru;
    if (!cur.has_next) {
      if (!cur.rows_change) fail(c, HV, order, "last pair does not flush", cur.ru, cur.J);
      if (cur.v_next < cur.total()) fail(c, HV, order, "walk ends before its claimed unit", cur.v_next, cur.total());
      if (flush_ru >= 0) flush();
      done = true;
      return;
    }
    const int ru = cur.ru, sl = cur.slice, nru = cur.next_ru(), nJ = cur.next_J, nsl = cur.next_slice();
    const bool announced = cur.rows_change, opens = cur.new_unit;
    const bool changed = cur.advance();
    if (cur.ru != nru || cur.J != nJ || cur.slice != nsl) fail(c, HV, order, "advance differs from peek", cur.ru, cur.J);
    if (changed != announced || changed != (cur.ru != ru || cur.slice != sl))
      fail(c, HV, order, "rows change", ru, cur.ru);
    if (cur.new_unit != opens) fail(c, HV, order, "new_unit changed by advance", ru, cur.ru);
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

template <int HV>
void run_case(const Case& c, int order) {
  const int nj2 = 2 * c.ns;
  Launch L;
  L.G = c.G;
  L.counted = order != kStatic && !c.contig;
  if (order == kCounterPastEnd) L.next = 1u << 20;  // whatever the counter holds: every claim is past the end
  L.visits.assign(static_cast<size_t>(c.n_slices) * (c.ns + 2) * nj2, 0);
  int64_t chunk_j = c.j_hi - c.j_lo, n_chunks = 1;
  if (!c.contig) column_chunks(c.j_hi - c.j_lo, c.nc, &chunk_j, &n_chunks);
  std::vector<Block<HV>> blocks;
  blocks.reserve(c.G);
  for (int g = 0; g < c.G; ++g)
    blocks.emplace_back(c, L, order, static_cast<int>(chunk_j), static_cast<int>(n_chunks), g);
  int live = c.G;
  int64_t steps = 0;
  const int64_t max_steps = int64_t{4} * c.n_slices * (c.ns + 2) * nj2 + 8 * c.G + 64;
  while (live > 0 && steps <= max_steps) {
    for (int g = 0; g < c.G && live > 0; ++g) {
      Block<HV>& b = order == kRandom ? blocks[rnd() % c.G] : blocks[g];
      if (b.done) continue;
      do {
        b.step();
        ++steps;
      } while (order == kOneTakesAll && !b.done && steps <= max_steps);
      if (b.done) --live;
    }
  }
  if (live > 0) return fail(c, HV, order, "walk does not end", live, static_cast<int>(steps));
  if (order == kCounterPastEnd) {
    // every block walked the unit it entered by itself and nothing else
    for (const auto& b : blocks)
      if (b.n_units > 1) fail(c, HV, order, "unit entered from a claim past the end", b.n_units, 0);
    for (int v : L.visits)
      if (v > 1) fail(c, HV, order, "pair visited twice", v, 0);
    return;
  }
  for (int sl = 0; sl < c.n_slices; ++sl)
    for (int P = 0; P < c.ns + 2; ++P)
      for (int J = 0; J < nj2; ++J)
        if (L.visits[(static_cast<size_t>(sl) * (c.ns + 2) + P) * nj2 + J] != (expected(c, P, J) ? 1 : 0))
          fail(c, HV, order, "visits", P, J);
}

int sweep() {
  int64_t cases = 0;
  for (int ns = 1; ns <= 9; ++ns)
    for (int srow0 = 0; srow0 < ns; srow0 += 2)
      for (int n_srb : {ns - srow0 + 1, (ns - srow0 + 1) / 2})
        for (int j_lo = 0; j_lo < 2 * ns; j_lo += 5)
          for (int j_hi : {2 * ns, j_lo + (2 * ns - j_lo + 1) / 2}) {
            if (n_srb < 1 || j_hi <= j_lo) continue;
            const int skips[2][2] = {{0, 0}, {j_lo + 1, j_lo + 3}};
            for (const auto& sk : skips)
              for (int G : {1, 3, 5, 7})
                for (int n_slices = 1; n_slices <= 3; ++n_slices) {
                  Case c{ns, srow0, n_srb, j_lo, j_hi, sk[0], sk[1], G, 0, 1, n_slices};
                  for (int nc = 1; nc <= 4; ++nc) {
                    c.nc = nc;
                    for (int order : {kTurns, kOneTakesAll, kRandom, kStatic, kCounterPastEnd}) {
                      run_case<1>(c, order);
                      run_case<2>(c, order);
                      cases += 2;
                    }
                  }
                  if (n_slices == 1) {  // the contiguous form walks through the same cursor (fixed deal)
                    c.contig = 1;
                    c.nc = 1;
                    run_case<1>(c, kStatic);
                    ++cases;
                  }
                }
          }
  printf("cases %lld failures %d\n", static_cast<long long>(cases), g_failures);
  return g_failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
  fprintf(stderr, "usage: %s sweep\n", argv[0]);
  return 2;
}
