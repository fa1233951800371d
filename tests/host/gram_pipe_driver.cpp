// CPU driver of the wide form's pair loop as of round 12 (gram_csym_kernel<128,
// 8, 4>: the look-ahead of each wave at lookahead_tiles() column tiles into the
// pair, and GramSchedule<4>::first_r's closed form away from the diagonal) for
// tests/test_gram_pipe_schedule.py.  It runs every wave of every block through
// the kernel's loop -- GramClaimCursor<4> as the kernel drives it -- with the
// MFMAs replaced by the chains they form: a chain is (sub-slice, row super
// block P, column block J, wave of the half, group of eight row tiles).  The
// model keeps the two ring buffers (the barrier count at each DMA and read),
// the two claim words (the barrier count at each write and read), the block's
// row accumulator (which rows-instance its sums belong to) and every wave's
// barrier count.  Events of one wave between two barriers are ordered; events
// of different waves are ordered only by a barrier between them, so every
// check compares barrier counts.
//   driver sweep   a thinned sweep of gram_schedule_wide_driver.cpp's, under
//                  the fixed deal and two orders of the claims; prints
//                  "cases N failures M"
//   driver kinds NS SROW0 N_SRB J_LO J_HI SKIP_LO SKIP_HI G0 MIN_CHUNKS N_SUB
//                  one launch planned with plan_launch<4> as the launcher
//                  does; prints the count of every boundary kind and
//                  "failures M"
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

int owner(int P, int Q) {
  if (P == Q) return P;
  const int lo = P < Q ? P : Q, hi = P < Q ? Q : P;
  return (P + Q) % 2 == 0 ? lo : hi;
}

struct Case {
  int ns, srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi, G, chunk_j, n_chunks, n_slices;
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
    printf("FAIL %s (%d, %d): ns %d srow0 %d n_srb %d j [%d, %d) skip [%d, %d) G %d chunk_j %d slices %d order %d\n",
           what, a, b, c.ns, c.srow0, c.n_srb, c.j_lo, c.j_hi, c.skip_lo, c.skip_hi, c.G, c.chunk_j, c.n_slices,
           order);
}

// first_r against the rule restated: the first raw column of [r, rhi) whose
// column block some live super block of the row unit owns and no skip range holds
void check_first_r(const Case& c) {
  const GramSchedule<HV> s(c.srow0, c.n_srb, c.j_lo, c.j_hi, c.skip_lo, c.skip_hi, c.ns, c.chunk_j, c.n_chunks, 0, c.G,
                           0);
  const int nj = c.j_hi - c.j_lo;
  for (int ru = 0; ru < s.n_ru; ++ru)
    for (int rhi : {nj, nj / 2 + 1})
      for (int r = 0; r <= rhi; ++r) {
        int want = -1;
        for (int q = r; q < rhi && want < 0; ++q)
          for (int h = 0; h < HV; ++h)
            if (expected(c, c.srow0 + 8 * (ru >> 1) + (ru & 1) + 2 * h, c.j_lo + q)) want = q;
        if (s.first_r(ru, r, rhi) != want) fail(c, -1, "first_r", ru, r);
      }
}

// each SIMD's two waves (w, w + 4) run their look-ahead at different places of the pair, one of them at its start
void check_lookahead_tiles() {
  const Case none{};
  for (int w = 0; w < kWaves / 2; ++w) {
    const int a = lookahead_tiles(w, kWaves, kStagger), b = lookahead_tiles(w + kWaves / 2, kWaves, kStagger);
    if (a != 0 || b <= 0 || b >= kTiles) fail(none, -1, "lookahead_tiles", a, b);
  }
}

struct Kinds {
  long long same_rows = 0, rows_change = 0, sub_slice = 0, one_pair_unit = 0, act_to_idle = 0, idle_to_act = 0,
            single_pair_block = 0, claim_past_end = 0;
};

struct Launch {
  unsigned next = 0;
  bool counted = true;
  int G = 1;
  std::vector<int> folds;  // [sub-slice][P][J][wave of the half][group]
  Kinds kinds;
};

// A block, one pair per step(): the kernel's pair loop.  The cursor's values
// are the same in every wave (each wave keeps its own copy and runs the same
// calls on it), so the model keeps one and notes, per wave, when it ran them.
struct Block {
  const Case& c;
  Launch& L;
  int order;
  GramSchedule<HV> sched;
  GramClaimCursor<HV> cur;
  bool done = false, started = false;
  int claim_word[2] = {-1, -1}, claim_par = 0;
  int word_write_epoch[2] = {-1, -1}, word_read_epoch[2] = {-1, -1};
  int buf = 0, flush_ru = -1, flush_inst = -1;
  int inst = 0;             // rows-instance (row unit x sub-slice visit) of the current pair
  int flushed_upto = -1;    // the last rows-instance flushed
  int max_fold_inst = -1;   // the latest rows-instance with a sum in rowacc
  int epoch = 0;            // barriers executed
  int barriers[kWaves] = {};
  int dma_epoch[2] = {-1, -1}, read_epoch[2] = {-1, -1};
  int pairs = 0, pairs_in_inst = 0;

  Block(const Case& c_, Launch& L_, int order_, int g)
      : c(c_), L(L_), order(order_),
        sched(c_.srow0, c_.n_srb, c_.j_lo, c_.j_hi, c_.skip_lo, c_.skip_hi, c_.ns, c_.chunk_j, c_.n_chunks, 0, c_.G, g),
        cur(sched, c_.n_slices) {}

  void barrier() {  // (every wave runs the loop's and claim_take()'s barriers, wherever its look-ahead sits)
    ++epoch;
    for (int& b : barriers) ++b;
  }
  // lane 0's claim: written to the word of the next claim
  void claim_begin() {
    if (!L.counted) return;
    // every wave's read of the word's last value lies before a barrier behind us
    if (word_read_epoch[claim_par] >= epoch) fail(c, order, "claim word written in the epoch of its read", claim_par, epoch);
    claim_word[claim_par] = L.G + static_cast<int>(L.next++);
    word_write_epoch[claim_par] = epoch;
  }
  int claim_end(int last) {
    int u = cur.static_next(last);
    if (L.counted) {
      if (word_write_epoch[claim_par] < 0 || word_write_epoch[claim_par] >= epoch)
        fail(c, order, "claim read before the barrier behind its write", claim_par, epoch);
      u = claim_word[claim_par];
      word_read_epoch[claim_par] = epoch;  // (some wave reads it as late as its look-ahead: anywhere in this epoch)
    }
    claim_par ^= 1;
    return u;
  }
  void claim_take() {
    while (!cur.claimed(claim_end(cur.v_next))) {
      claim_begin();
      if (L.counted) barrier();
    }
  }
  void dma(int b) {
    // the buffer's last read by any wave lies before a barrier every wave has passed
    if (read_epoch[b] >= epoch) fail(c, order, "DMA into a buffer read since the last barrier", b, epoch);
    dma_epoch[b] = epoch;  // (the late waves' pieces: anywhere in this epoch)
  }
  void fold(int sl, int P, int J, int w4, int grp) {
    const int nj2 = 2 * c.ns;
    if (P < 0 || P >= p_rows(c) || J < 0 || J >= nj2 || sl < 0 || sl >= c.n_slices)
      return fail(c, order, "fold out of range", P, J);
    ++L.folds[(((static_cast<size_t>(sl) * p_rows(c) + P) * nj2 + J) * kWPS + w4) * 2 + grp];
    if (inst <= flushed_upto) fail(c, order, "fold behind its unit's flush", P, J);
    if (inst < max_fold_inst) fail(c, order, "fold behind a later unit's first fold", P, J);
    if (inst > max_fold_inst) max_fold_inst = inst;
  }
  void flush() {
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
    dma_epoch[0] = epoch;  // issue(0, ...) before the loop's first barrier
    claim_begin();
  }
  void step() {
    if (!started) return start();
    bool act[kWaves], any_act = false;
    for (int w = 0; w < kWaves; ++w) any_act |= act[w] = cur.acts(w / kWPS);  // (before the barrier, the current pair)
    barrier();
    if (flush_ru >= 0) flush();  // every wave, behind the barrier, before its column tiles
    // the pair's column tiles read buf; every wave's look-ahead lies somewhere among them
    if (!any_act) fail(c, order, "pair no part acts on", cur.ru, cur.J);
    if (dma_epoch[buf] < 0 || dma_epoch[buf] >= epoch) fail(c, order, "read before the barrier behind the DMA", buf, epoch);
    for (int w = 0; w < kWaves; ++w) {
      const int t = act[w] ? lookahead_tiles(w, kWaves, kStagger) : 0;
      if (t < 0 || t >= kTiles) fail(c, order, "look-ahead outside the pair", w, t);
    }
    // the look-ahead (one cursor for all waves, see above)
    const bool fresh_claim = cur.new_unit;
    if (cur.new_unit) claim_take();
    cur.peek();
    if (cur.has_next) dma(buf ^ 1);
    if (fresh_claim && !cur.has_next && pairs == 0) ++L.kinds.claim_past_end;
    read_epoch[buf] = epoch;
    // the chains: folded behind the pair's last MFMA, before the next barrier
    const bool same_rows_next = cur.has_next && !cur.rows_change;
    bool any_both = false;
    for (int w = 0; w < kWaves; ++w) {
      const int half = w / kWPS;
      const bool acts_next = same_rows_next && sched.takes_h(cur.next_ru(), half, cur.next_J);
      if (act[w]) {
        for (int grp = 0; grp < 2; ++grp) fold(cur.slice, sched.rowP(cur.ru, half), cur.J, w % kWPS, grp);
        if (acts_next) any_both = true;
        if (same_rows_next && !acts_next) ++L.kinds.act_to_idle;
      } else if (acts_next) {
        ++L.kinds.idle_to_act;
      }
    }
    ++pairs;
    ++pairs_in_inst;
    buf ^= 1;
    if (cur.rows_change) {
      flush_ru = cur.ru;
      flush_inst = inst;
      if (pairs_in_inst == 1) ++L.kinds.one_pair_unit;
    }
    if (!cur.has_next) {
      if (!cur.rows_change) fail(c, order, "last pair does not flush", cur.ru, cur.J);
      if (cur.v_next < cur.total()) fail(c, order, "walk ends before its claimed unit", cur.v_next, cur.total());
      if (pairs == 1) ++L.kinds.single_pair_block;
      barrier();
      flush();
      for (int w = 1; w < kWaves; ++w)
        if (barriers[w] != barriers[0]) fail(c, order, "waves differ in their barriers", w, 0);
      done = true;
      return;
    }
    if (cur.rows_change) {
      if (cur.next_ru() == cur.ru) ++L.kinds.sub_slice; else ++L.kinds.rows_change;
    } else if (any_both) {
      ++L.kinds.same_rows;
    }
    if (cur.advance()) {
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
            fail(c, order, "chain not folded exactly once", P, J);
  if (kinds) *kinds = L.kinds;
}

int sweep() {
  int64_t cases = 0;
  check_lookahead_tiles();
  for (int ns : {1, 2, 3, 5, 8, 9, 13, 17})
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
                  for (int n_sub : {2, 4}) {
                    int64_t cj, nch;
                    column_chunks(j_hi - j_lo, nc, &cj, &nch);
                    const Case c{ns, srow0, n_srb, j_lo, j_hi, sk[0], sk[1], G, static_cast<int>(cj),
                                 static_cast<int>(nch), n_sub};
                    if (G == 1 && n_sub == 2) check_first_r(c);
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
  if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc == 12 && !strcmp(argv[1], "kinds")) {
    int v[10];
    for (int i = 0; i < 10; ++i) v[i] = atoi(argv[2 + i]);
    const GramLaunch L = plan_launch<HV>(v[1], v[2], v[3], v[4], v[5], v[6], v[0], v[7], 0, v[8], v[9]);
    if (L.G <= 0) {
      printf("no work\n");
      return 1;
    }
    const Case c{v[0], v[1], v[2], v[3], v[4], v[5], v[6], L.G, L.chunk_j, L.n_chunks, v[9]};
    check_first_r(c);
    Kinds k;
    run(c, L.units > L.G ? kTurns : kStatic, &k);
    printf("G %d chunks %d same_rows %lld rows_change %lld sub_slice %lld one_pair_unit %lld act_to_idle %lld "
           "idle_to_act %lld single_pair_block %lld claim_past_end %lld failures %d\n",
           L.G, L.n_chunks, k.same_rows, k.rows_change, k.sub_slice, k.one_pair_unit, k.act_to_idle, k.idle_to_act,
           k.single_pair_block, k.claim_past_end, g_failures);
    return g_failures ? 1 : 0;
  }
  fprintf(stderr, "usage: %s sweep | kinds NS SROW0 N_SRB J_LO J_HI SKIP_LO SKIP_HI G0 MIN_CHUNKS N_SUB\n", argv[0]);
  return 2;
}
