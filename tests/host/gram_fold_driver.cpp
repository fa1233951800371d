// CPU driver of the integer forms' pair loop as of round 15 (gram_i8sym_kernel
// and gram_fp4sym_kernel: the wide form over whole slices, whose row chains run
// over up to Cfg::FOLD_PAIRS pairs of a row unit before they are folded) for
// tests/test_gram_fold_schedule.py.  It runs every wave of every block through
// the kernel's loop -- GramClaimCursor<4>, lookahead_tiles() and fold_due() of
// gram_schedule.hpp, as the kernel calls them -- with the MFMAs replaced by
// the contributions they add to the wave's chain: (slice, row super block P,
// column block J).  A fold hands the chain's contributions to the block's row
// accumulator; the model notes which rows-instance they belong to, when the
// accumulator was flushed and when the resident rows were replaced.
// (tests/host/gram_pipe_driver.cpp keeps modelling the fp16 form, with its
// ring buffers and claim words; they are the same here and are not repeated.)
//   driver sweep R   a thinned sweep under the fixed deal and two orders of the
//                    claims, chains of up to R pairs; prints "cases N failures M"
//   driver kinds R NS SROW0 N_SRB J_LO J_HI SKIP_LO SKIP_HI G0 MIN_CHUNKS N_SLICES
//                    one launch planned with plan_launch<4> as the launcher
//                    does; prints the count of every fold trigger and
//                    "failures M"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "gram_schedule.hpp"

using namespace dal;

namespace {

constexpr int HV = 4, kWaves = 8, kWPS = 2;  // waves per block, per half
constexpr int kTiles = 16;                   // column tiles of a pair
constexpr int kStagger = 4;                  // DAL_GRAM_STAGGER's default
constexpr int kMaxR = 32;

int owner(int P, int Q) {
  if (P == Q) return P;
  const int lo = P < Q ? P : Q, hi = P < Q ? Q : P;
  return (P + Q) % 2 == 0 ? lo : hi;
}

struct Case {
  int ns, srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi, G, chunk_j, n_chunks, n_slices, R;
};
enum Order { kTurns, kRandom, kStatic };

bool expected(const Case& c, int P, int J) {
  return P >= c.srow0 && P < c.srow0 + c.n_srb && P < c.ns && J >= c.j_lo && J < c.j_hi &&
         !(J >= c.skip_lo && J < c.skip_hi) && owner(P, J / 2) == P;
}
int p_rows(const Case& c) { return c.ns + 2 * HV + 2; }

int g_failures = 0;
void fail(const Case& c, int order, const char* what, int a, int b) {
  if (++g_failures <= 20)
    printf("FAIL %s (%d, %d): R %d ns %d srow0 %d n_srb %d j [%d, %d) skip [%d, %d) G %d chunk_j %d slices %d order %d\n",
           what, a, b, c.R, c.ns, c.srow0, c.n_srb, c.j_lo, c.j_hi, c.skip_lo, c.skip_hi, c.G, c.chunk_j, c.n_slices,
           order);
}

// the fold triggers (per wave and fold)
struct Kinds {
  long long cap = 0;                  // the chain holds R pairs
  long long partial[kMaxR] = {};      // a rows change with p pairs pending, 1 <= p < R
  long long idle_fold = 0;            // a rows change while the wave idles with a pending chain
  long long span_idle = 0;            // a chain takes a pair behind one its wave idled on
  long long one_pair_unit = 0;        // a rows-instance of a single pair, folded
  long long same_rows_slice = 0;      // the rows change to another slice of the same row unit
  long long walk_end = 0;             // the fold at the block's last pair
  long long folds = 0, pairs = 0;
};

struct Contribution {
  int slice, P, J;
};

struct Launch {
  unsigned next = 0;
  bool counted = true;
  int G = 1;
  std::vector<int> folds;  // [slice][P][J][wave of the half][group of eight row tiles]
  Kinds kinds;
};

// A block, one pair per step(): the kernel's pair loop.  The cursor's values
// are the same in every wave, so the model keeps one; the chains, their pair
// counts and the barriers are per wave.
struct Block {
  const Case& c;
  Launch& L;
  int order;
  GramSchedule<HV> sched;
  GramClaimCursor<HV> cur;
  bool done = false, started = false;
  int claim_word[2] = {-1, -1}, claim_par = 0;
  int flush_ru = -1, flush_inst = -1;
  int inst = 0;             // rows-instance (row unit x slice visit) of the current pair
  int flushed_upto = -1;    // the last rows-instance flushed
  int max_fold_inst = -1;   // the latest rows-instance with a sum in rowacc
  int barriers[kWaves] = {};
  int pending[kWaves] = {};           // the kernel's counter
  bool idled[kWaves] = {};            // the wave idled on a pair with its chain pending
  int chain_inst[kWaves] = {};
  std::vector<Contribution> chain[kWaves];
  int pairs = 0, pairs_in_inst = 0;

  Block(const Case& c_, Launch& L_, int order_, int g)
      : c(c_), L(L_), order(order_),
        sched(c_.srow0, c_.n_srb, c_.j_lo, c_.j_hi, c_.skip_lo, c_.skip_hi, c_.ns, c_.chunk_j, c_.n_chunks, 0, c_.G, g),
        cur(sched, c_.n_slices) {}

  void barrier() {
    for (int& b : barriers) ++b;
  }
  void claim_begin() {
    if (!L.counted) return;
    claim_word[claim_par] = L.G + static_cast<int>(L.next++);
  }
  int claim_end(int last) {
    int u = cur.static_next(last);
    if (L.counted) u = claim_word[claim_par];
    claim_par ^= 1;
    return u;
  }
  void claim_take() {
    while (!cur.claimed(claim_end(cur.v_next))) {
      claim_begin();
      if (L.counted) barrier();
    }
  }
  // fold_rows() of wave w: its chain goes to the block's row accumulator
  void fold(int w) {
    const int nj2 = 2 * c.ns;
    if (chain[w].empty() || static_cast<int>(chain[w].size()) != pending[w])
      fail(c, order, "fold of a chain that does not hold its pending pairs", w, pending[w]);
    for (const Contribution& k : chain[w]) {
      if (k.P < 0 || k.P >= p_rows(c) || k.J < 0 || k.J >= nj2 || k.slice < 0 || k.slice >= c.n_slices) {
        fail(c, order, "fold out of range", k.P, k.J);
        continue;
      }
      if (k.P != sched.rowP(cur.ru, w / kWPS) || k.slice != cur.slice)
        fail(c, order, "chain folded into other rows than it was formed on", k.P, k.J);
      for (int grp = 0; grp < 2; ++grp)
        ++L.folds[(((static_cast<size_t>(k.slice) * p_rows(c) + k.P) * nj2 + k.J) * kWPS + w % kWPS) * 2 + grp];
    }
    if (chain_inst[w] != inst) fail(c, order, "chain folded in a later rows-instance", chain_inst[w], inst);
    if (inst <= flushed_upto) fail(c, order, "fold behind its unit's flush", w, inst);
    if (inst < max_fold_inst) fail(c, order, "fold behind a later unit's first fold", w, inst);
    if (inst > max_fold_inst) max_fold_inst = inst;
    chain[w].clear();
    pending[w] = 0;
    idled[w] = false;
    ++L.kinds.folds;
  }
  void flush() {
    for (int w = 0; w < kWaves; ++w)
      if (pending[w] != 0) fail(c, order, "flush while a wave holds a chain", w, pending[w]);
    if (max_fold_inst > flush_inst) fail(c, order, "flush of rows holding a later unit's sums", flush_ru, max_fold_inst);
    flushed_upto = flush_inst;
    flush_ru = flush_inst = -1;
  }
  void start() {
    started = true;
    if (!cur.claimed(cur.first_unit())) {
      claim_begin();
      if (L.counted) barrier();
      claim_take();
    }
    if (!cur.start()) {
      done = true;
      return;
    }
    claim_begin();
  }
  void step() {
    if (!started) return start();
    bool act[kWaves], any_act = false;
    for (int w = 0; w < kWaves; ++w) any_act |= act[w] = cur.acts(w / kWPS);  // (before the barrier, the current pair)
    barrier();
    if (flush_ru >= 0) flush();  // every wave, behind the barrier, before its column tiles
    if (!any_act) fail(c, order, "pair no part acts on", cur.ru, cur.J);
    for (int w = 0; w < kWaves; ++w) {
      const int t = act[w] ? lookahead_tiles(w, kWaves, kStagger) : 0;
      if (t < 0 || t >= kTiles) fail(c, order, "look-ahead outside the pair", w, t);
    }
    // the look-ahead: every wave has run it when it reaches the end of the pair's body
    if (cur.new_unit) claim_take();
    cur.peek();
    ++pairs;
    ++pairs_in_inst;
    ++L.kinds.pairs;
    const bool slice_of_same_rows = cur.rows_change && cur.has_next && cur.next_ru() == cur.ru;
    for (int w = 0; w < kWaves; ++w) {
      if (act[w]) {
        if (pending[w] == 0) chain_inst[w] = inst;
        if (pending[w] > 0 && idled[w]) {
          ++L.kinds.span_idle;
          idled[w] = false;
        }
        chain[w].push_back({cur.slice, sched.rowP(cur.ru, w / kWPS), cur.J});
        ++pending[w];
        if (pending[w] > c.R) fail(c, order, "chain of more than FOLD_PAIRS pairs", w, pending[w]);
      } else if (pending[w] > 0) {
        idled[w] = true;
      }
      // the end of the pair's body, before the barrier
      if (fold_due(pending[w], c.R, cur.rows_change)) {
        if (pending[w] >= c.R) {
          ++L.kinds.cap;
        } else {
          ++L.kinds.partial[pending[w]];
        }
        if (cur.rows_change) {
          if (!act[w]) ++L.kinds.idle_fold;
          if (pairs_in_inst == 1) ++L.kinds.one_pair_unit;
          if (slice_of_same_rows) ++L.kinds.same_rows_slice;
          if (!cur.has_next) ++L.kinds.walk_end;
        }
        fold(w);
      }
    }
    if (cur.rows_change) {
      flush_ru = cur.ru;
      flush_inst = inst;
    }
    if (!cur.has_next) {
      if (!cur.rows_change) fail(c, order, "last pair does not flush", cur.ru, cur.J);
      if (cur.v_next < cur.total()) fail(c, order, "walk ends before its claimed unit", cur.v_next, cur.total());
      barrier();
      flush();
      for (int w = 1; w < kWaves; ++w)
        if (barriers[w] != barriers[0]) fail(c, order, "waves differ in their barriers", w, 0);
      done = true;
      return;
    }
    if (cur.advance()) {  // load_a replaces the resident rows
      for (int w = 0; w < kWaves; ++w)
        if (pending[w] != 0) fail(c, order, "rows replaced under a pending chain", w, pending[w]);
      ++inst;
      pairs_in_inst = 0;
    }
    if (cur.new_unit) claim_begin();
  }
};

unsigned g_rng = 12345u;
unsigned rnd() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng >> 8;
}

void run(const Case& c, int order, Kinds* kinds) {
  const int nj2 = 2 * c.ns;
  Launch L;
  L.G = c.G;
  L.counted = order != kStatic;
  L.folds.assign(static_cast<size_t>(c.n_slices) * p_rows(c) * nj2 * kWPS * 2, 0);
  std::vector<Block> blocks;
  blocks.reserve(c.G);
  for (int g = 0; g < c.G; ++g) blocks.emplace_back(c, L, order, g);
  int live = c.G;
  int64_t steps = 0;
  const int64_t max_steps = int64_t{4} * c.n_slices * p_rows(c) * nj2 + 8 * c.G + 64;
  while (live > 0 && steps <= max_steps) {
    for (int g = 0; g < c.G && live > 0; ++g) {
      Block& b = order == kRandom ? blocks[rnd() % c.G] : blocks[g];
      if (b.done) continue;
      b.step();
      ++steps;
      if (b.done) --live;
    }
  }
  if (live > 0) return fail(c, order, "walk does not end", live, static_cast<int>(steps));
  for (int sl = 0; sl < c.n_slices; ++sl)
    for (int P = 0; P < p_rows(c); ++P)
      for (int J = 0; J < nj2; ++J)
        for (int k = 0; k < kWPS * 2; ++k)
          if (L.folds[((static_cast<size_t>(sl) * p_rows(c) + P) * nj2 + J) * kWPS * 2 + k] !=
              (expected(c, P, J) ? 1 : 0))
            fail(c, order, "contribution not folded exactly once", P, J);
  if (kinds) *kinds = L.kinds;
}

int sweep(int R) {
  int64_t cases = 0;
  for (int ns : {1, 2, 3, 5, 8, 9, 13, 17, 33})
    for (int srow0 : {0, 1, ns / 2}) {
      if (srow0 >= ns || (srow0 == 1 && ns / 2 == 1)) continue;
      for (int n_srb : {ns - srow0 + 1, ns - srow0, (ns - srow0 + 1) / 2}) {
        if (n_srb < 1) continue;
        for (int j_lo = 0; j_lo < 2 * ns; j_lo += 7)
          for (int j_hi : {2 * ns, j_lo + (2 * ns - j_lo + 1) / 2}) {
            if (j_hi <= j_lo) continue;
            const int skips[3][2] = {{0, 0}, {2 * srow0, 2 * (srow0 + n_srb)}, {j_lo + 1, j_lo + 3}};
            for (const auto& sk : skips)
              for (int G : {1, 3, 7})
                for (int nc : {1, 3})
                  for (int n_sl : {1, 2}) {
                    int64_t cj, nch;
                    column_chunks(j_hi - j_lo, nc, &cj, &nch);
                    const Case c{ns, srow0, n_srb, j_lo, j_hi, sk[0], sk[1], G, static_cast<int>(cj),
                                 static_cast<int>(nch), n_sl, R};
                    for (int order : {kStatic, kTurns, kRandom}) {
                      run(c, order, nullptr);
                      ++cases;
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
  const int R = argc >= 3 ? atoi(argv[2]) : 0;
  if (argc >= 3 && (R < 1 || R >= kMaxR)) {
    fprintf(stderr, "R out of range\n");
    return 2;
  }
  if (argc == 3 && !strcmp(argv[1], "sweep")) return sweep(R);
  if (argc == 13 && !strcmp(argv[1], "kinds")) {
    int v[10];
    for (int i = 0; i < 10; ++i) v[i] = atoi(argv[3 + i]);
    const GramLaunch L = plan_launch<HV>(v[1], v[2], v[3], v[4], v[5], v[6], v[0], v[7], 0, v[8], v[9]);
    if (L.G <= 0) {
      printf("no work\n");
      return 1;
    }
    const Case c{v[0], v[1], v[2], v[3], v[4], v[5], v[6], L.G, L.chunk_j, L.n_chunks, v[9], R};
    Kinds k;
    run(c, L.units > L.G ? kTurns : kStatic, &k);
    long long partial = 0;
    int partial_kinds = 0;
    for (int p = 1; p < R; ++p) {
      partial += k.partial[p];
      partial_kinds += k.partial[p] > 0;
    }
    printf("G %d chunks %d pairs %lld folds %lld cap %lld partial %lld partial_kinds %d idle_fold %lld span_idle %lld "
           "one_pair_unit %lld same_rows_slice %lld walk_end %lld failures %d\n",
           L.G, L.n_chunks, k.pairs, k.folds, k.cap, partial, partial_kinds, k.idle_fold, k.span_idle, k.one_pair_unit,
           k.same_rows_slice, k.walk_end, g_failures);
    for (int p = 1; p < R; ++p) printf("partial_%d %lld ", p, k.partial[p]);
    printf("\n");
    return g_failures ? 1 : 0;
  }
  fprintf(stderr, "usage: %s sweep R | kinds R NS SROW0 N_SRB J_LO J_HI SKIP_LO SKIP_HI G0 MIN_CHUNKS N_SLICES\n",
          argv[0]);
  return 2;
}
