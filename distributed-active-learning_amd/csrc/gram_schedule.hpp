// The pair schedule of the symmetric Gram (gram_sym.hip): which block
// multiplies which (512-row super block P, 256-column block J) pair, in what
// order, and when a row unit's sums are flushed.  Integer arithmetic only, no
// HIP header: gram_csym_kernel and its launcher both use this file, and
// tests/test_gram_schedule.py walks it on the CPU (tests/host/
// gram_schedule_driver.cpp) against an independent statement of the rule.
#pragma once

#include <stdint.h>

#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define DAL_HD __host__ __device__ __forceinline__
#else
#define DAL_HD inline
#endif

namespace dal {

// The orientation rule: each unordered pair {P, Q} of super blocks is
// multiplied once, by its taker.  P takes Q iff Q == P (diagonal), Q > P with
// P + Q even, or Q < P with P + Q odd (global indices, so the bits do not
// depend on the sharding).
template <class I>
DAL_HD bool sb_takes(I P, I Q) {
  return Q == P || (Q > P && ((P + Q) & 1) == 0) || (Q < P && ((P + Q) & 1));
}

// One launch of gram_csym_kernel as block g of G sees it.  Work = the pairs
// (P, J) over row super blocks P and 256-column blocks J in [j_lo, j_hi) minus
// [skip_lo, skip_hi), as segments (row unit, raw column range [rlo, rhi))
// walked by a raw column cursor r (J = jmap(r)).  A row unit is one super
// block (HV = 1) or HV of the same parity out of 2 HV consecutive ones, P,
// P + 2, ... (HV = 2, 4: they take the same column blocks but near the
// diagonal, so one B stage feeds all; a part whose super block does not take J
// idles):
//  contig: block g owns the g-th 1/G of the unit-major raw grid (HV = 1 only:
//          form_ok);
//  chunk:  unit u = (row unit u % n_ru, column chunk u / n_ru), dealt round-robin
//          (all blocks sweep the same column chunks together: L2 / MALL reuse);
//          the kernel takes the units beyond each block's first from a counter
//          instead, over every feature slice in one launch (GramClaimCursor).
template <int HV>
struct GramSchedule {
  static_assert(HV == 1 || HV == 2 || HV == 4, "one, two or four super blocks per row unit");
  // the contiguous form indexes its segments by super block, not by row unit
  static constexpr bool form_ok(int contig) { return HV == 1 || !contig; }

  int srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi, ns_active, chunk_j, n_chunks, contig, G, g;
  int n_ru;         // row units of the launch
  int sk_lo, skl;   // the skip range clamped to the columns; its length (contig; chunk mode skips through takes())
  int nje;          // raw columns per row: the columns less the clamped skip range
  int nre;          // live row super blocks
  int64_t ka, kb;   // contig: this block's share [ka, kb) of the raw grid
  int n_seg;        // segments: this block's (contig) or the launch's units (chunk)

  DAL_HD GramSchedule(int srow0_, int n_srb_, int j_lo_, int j_hi_, int skip_lo_, int skip_hi_, int ns_active_,
                      int chunk_j_, int n_chunks_, int contig_, int G_ = 1, int g_ = 0)
      : srow0(srow0_), n_srb(n_srb_), j_lo(j_lo_), j_hi(j_hi_), skip_lo(skip_lo_), skip_hi(skip_hi_),
        ns_active(ns_active_), chunk_j(chunk_j_), n_chunks(n_chunks_), contig(contig_), G(G_), g(g_) {
    n_ru = HV == 1 ? n_srb : 2 * ((n_srb + 2 * HV - 1) / (2 * HV));
    sk_lo = skip_lo > j_lo ? skip_lo : j_lo;
    const int sk_hi = skip_hi < j_hi ? skip_hi : j_hi;
    skl = contig && sk_hi > sk_lo ? sk_hi - sk_lo : 0;
    nje = j_hi - j_lo - skl;
    const int nre0 = ns_active - srow0;
    nre = nre0 < n_srb ? (nre0 > 0 ? nre0 : 0) : n_srb;
    ka = raw() * g / G;
    kb = raw() * (g + 1) / G;
    n_seg = contig ? (kb > ka ? static_cast<int>((kb - 1) / nje - ka / nje) + 1 : 0) : n_units();
  }

  DAL_HD int64_t raw() const { return static_cast<int64_t>(nre) * nje; }  // contig: pairs dealt over the grid
  DAL_HD int n_units() const { return n_ru * n_chunks; }                  // chunk: units dealt over the grid
  DAL_HD int first_seg() const { return contig ? 0 : g; }
  DAL_HD int seg_step() const { return contig ? 1 : G; }

  DAL_HD int rowP(int ru, int h) const {
    return HV == 1 ? srow0 + ru : srow0 + 2 * HV * (ru >> 1) + (ru & 1) + 2 * h;
  }
  DAL_HD bool live(int P) const { return P < srow0 + n_srb && P < ns_active; }
  DAL_HD int seg_ru(int u) const { return contig ? static_cast<int>(ka / nje) + u : u % n_ru; }
  DAL_HD int seg_rlo(int u) const {
    return contig ? (u == 0 ? static_cast<int>(ka % nje) : 0) : (u / n_ru) * chunk_j;
  }
  DAL_HD int seg_rhi(int u) const {
    if (contig) return u == n_seg - 1 ? static_cast<int>((kb - 1) % nje) + 1 : nje;
    const int e = (u / n_ru + 1) * chunk_j;
    return e < nje ? e : nje;
  }
  DAL_HD int jmap(int r) const { return j_lo + r + (j_lo + r >= sk_lo ? skl : 0); }
  DAL_HD bool takes(int P, int J) const {
    if (J >= skip_lo && J < skip_hi) return false;
    return sb_takes(P, J >> 1);
  }
  // the unit's super block h takes J (and exists)
  DAL_HD bool takes_h(int ru, int h, int J) const { return live(rowP(ru, h)) && takes(rowP(ru, h), J); }
  DAL_HD bool takes_u(int ru, int J) const {
    for (int h = 0; h < HV; ++h)
      if (takes_h(ru, h, J)) return true;
    return false;
  }
  // the first raw column in [r, rhi) the unit takes, -1: none
  DAL_HD int first_r(int ru, int r, int rhi) const {
    if constexpr (HV == 1) {
      const int P = srow0 + ru;
      if (P >= ns_active) return -1;
      while (r < rhi && !takes(P, jmap(r))) ++r;
    } else {
      if (!live(rowP(ru, 0))) return -1;
      // Away from the unit's own super blocks P0 .. P0 + 2 HV - 2 every part lies
      // on one side of Q = J >> 1 and they share a parity, so takes_u is the
      // first (live) part's answer -- P0 + Q odd below the unit, even above it --
      // and an untaken Q is stepped over whole: two compares and a parity bit
      // per pair where the loop over the parts was ~100 scalar instructions,
      // run by all eight waves on the CU's one scalar unit behind every pair's
      // barrier (round 12).  Near the diagonal, in a skip range and in the
      // contiguous form the parts are asked one by one as before.
      const int P0 = rowP(ru, 0);
      while (r < rhi) {
        const int J = jmap(r), Q = J >> 1;
        if (skl == 0 && (Q < P0 || Q > P0 + 2 * HV - 2) && !(J >= skip_lo && J < skip_hi)) {
          if (((P0 + Q) & 1) == (Q < P0 ? 1 : 0)) break;
          r = 2 * (Q + 1) - j_lo;  // (skl == 0: jmap(r) is j_lo + r)
          continue;
        }
        if (takes_u(ru, J)) break;
        ++r;
      }
    }
    return r < rhi ? r : -1;
  }
  // the first segment from u on with work, and its first raw column (n_seg: none)
  DAL_HD int seek(int u, int& r) const {
    while (u < n_seg) {
      r = first_r(seg_ru(u), seg_rlo(u), seg_rhi(u));
      if (r >= 0) break;
      u += seg_step();
    }
    return u;
  }
};

// A block's walk over its pairs.  ru / J are the current pair's row unit and
// column block; peek() looks one pair ahead (the kernel prefetches next_J's
// first stage and flushes the row sums when rows_change) and advance() moves
// there.
template <int HV>
struct GramCursor {
  const GramSchedule<HV>& s;
  int unit = 0, r = -1, rhi_u = 0;  // segment, raw column in it, the segment's end
  int ru = -1, J = -1;
  // set by peek(); next_ru / next_J are -1 without a next pair
  int next_unit = 0, next_r = -1, next_ru = -1, next_J = -1;
  bool has_next = false, rows_change = false;

  DAL_HD explicit GramCursor(const GramSchedule<HV>& sched) : s(sched) {}
  // the block's first pair; false: the block has no work
  DAL_HD bool start() {
    unit = s.seek(s.first_seg(), r);
    if (unit >= s.n_seg) return false;
    ru = s.seg_ru(unit);
    rhi_u = s.seg_rhi(unit);
    J = s.jmap(r);
    return true;
  }
  DAL_HD void peek() {
    next_r = s.first_r(ru, r + 1, rhi_u);
    next_unit = unit;
    if (next_r < 0) next_unit = s.seek(unit + s.seg_step(), next_r);
    has_next = next_unit < s.n_seg;
    next_ru = has_next ? s.seg_ru(next_unit) : -1;
    rows_change = next_ru != ru;
    next_J = has_next ? s.jmap(next_r) : -1;
  }
  // to the pair peek() announced (has_next); true: the row unit changed
  DAL_HD bool advance() {
    unit = next_unit;
    rhi_u = s.seg_rhi(unit);
    ru = next_ru;
    r = next_r;
    J = next_J;
    return rows_change;
  }
  // half h's super block takes the current J?  (a half whose super block does not idles)
  DAL_HD bool acts(int h) const { return HV == 1 || s.takes_h(ru, h, J); }
};

// A block's walk over units it is handed one at a time (the kernel's walk
// since round 10).  A unit index names (feature slice, segment) -- the wide
// form (HV = 4) passes its 64-feature sub-slices as the slices --: the chunk
// form counts (slice * n_chunks + column chunk) * n_ru + row unit over every
// slice of the launch -- slice slowest, chunk next, so blocks that take
// consecutive indices sweep one column chunk together -- and the contiguous
// form counts the block's own segments of its one slice.  The cursor never
// decides which unit comes next: the block enters first_unit(), and whoever
// drives the walk hands over each later unit with claimed(), one unit ahead --
// from a counter shared by the launch's blocks (any order of the indices
// first_unit() .. total() - 1, each once over the launch, visits every pair
// once), or static_next() for the fixed deal of GramCursor.  An index at or
// beyond total() ends the walk; claimed() refuses a unit without a pair
// (claim again).  peek / advance / acts are GramCursor's.  new_unit: the
// current pair (after peek(): the announced one) is the first of its unit, so
// the unit behind it is to be claimed before the next peek().
// A unit index is taken apart once, when it is handed over (claimed() keeps
// the unit's slice, row unit, first taken column and end): peek() and
// advance() divide nothing, and the kernel holds few scalars beside the
// schedule's.
template <int HV>
struct GramClaimCursor {
  const GramSchedule<HV>& s;
  int n_slices;             // feature slices of the launch (contig: 1)
  // the claimed unit behind the current one: its index (>= total(): none) and,
  // if there is one (c_r >= 0), its slice, row unit, first taken raw column and end
  int v_next = -1, c_slice = -1, c_ru = -1, c_r = -1, c_rhi = 0;
  // the current pair
  int slice = 0, ru = -1, r = -1, rhi_u = 0, J = -1;
  // set by peek(): the next pair's raw column and column block (-1 without a next pair)
  int next_r = -1, next_J = -1;
  bool has_next = false, rows_change = false, new_unit = false;

  DAL_HD GramClaimCursor(const GramSchedule<HV>& sched, int n_slices_)
      : s(sched), n_slices(sched.contig ? 1 : n_slices_) {}
  DAL_HD int total() const { return s.contig ? s.n_seg : n_slices * s.n_units(); }
  DAL_HD int first_unit() const { return s.first_seg(); }
  DAL_HD int static_next(int u) const { return u + s.seg_step(); }
  // Hand over unit u as the one behind the current pair's.  false: u holds no
  // pair (nothing taken, skipped columns, rows past the pool) -- hand over
  // another one.  u >= total(): no unit follows.
  DAL_HD bool claimed(int u) {
    v_next = u;
    c_r = -1;
    if (u >= total()) return true;
    const int sg = s.contig ? u : u % s.n_units();
    c_slice = s.contig ? 0 : u / s.n_units();
    c_ru = s.seg_ru(sg);
    c_rhi = s.seg_rhi(sg);
    c_r = s.first_r(c_ru, s.seg_rlo(sg), c_rhi);
    return c_r >= 0;
  }
  // to the first pair of the unit handed over (the block's first); false: there is none
  DAL_HD bool start() {
    if (c_r < 0) return false;
    open();
    new_unit = true;
    return true;
  }
  DAL_HD int next_slice() const { return new_unit ? c_slice : slice; }
  DAL_HD int next_ru() const { return new_unit ? c_ru : ru; }
  DAL_HD void peek() {
    next_r = s.first_r(ru, r + 1, rhi_u);
    new_unit = next_r < 0;
    has_next = true;
    rows_change = false;
    if (new_unit) {
      has_next = c_r >= 0;
      next_r = c_r;
      // (another slice of the same rows restarts them too: one flag serves the A reload and the flush)
      rows_change = !has_next || c_ru != ru || c_slice != slice;
    }
    next_J = has_next ? s.jmap(next_r) : -1;
  }
  // to the pair peek() announced (has_next); true: the rows (row unit or slice) changed
  DAL_HD bool advance() {
    if (new_unit) {
      open();
    } else {
      r = next_r;
      J = next_J;
    }
    return rows_change;
  }
  DAL_HD bool acts(int h) const { return HV == 1 || s.takes_h(ru, h, J); }

 private:
  DAL_HD void open() {
    slice = c_slice;
    ru = c_ru;
    rhi_u = c_rhi;
    r = c_r;
    J = s.jmap(r);
  }
};

// Where the wide form's wave runs its look-ahead (round 12): the claim handed
// over, peek() and the DMA issue of the next pair's stage are scalar work no
// MFMA of the pair reads, ~1,300 cycles when the two waves of a SIMD (w and
// w + waves / 2, one program) run it at once behind the pair's barrier.  The
// first half of the block's waves runs it there, before the pair's column
// tiles; their SIMD partners run `stagger` column tiles first, so each wave's
// scalar work lies under its partner's MFMAs.  Returns the column tiles of
// the pair the wave multiplies before its look-ahead.  Every wave still runs
// it between the pair's barrier and the next one, so what the kernel's
// protocols need holds as before: the stage goes to the buffer every wave left
// before this barrier and has landed before the next, and a claim is read
// behind the barrier that follows its write and before the one that precedes
// the next write to its word (tests/test_gram_pipe_schedule.py walks this).
DAL_HD constexpr int lookahead_tiles(int wave, int waves, int stagger) { return wave < waves / 2 ? 0 : stagger; }

// When a wave of the integer forms folds its row chains (round 15).  A chain
// runs over the pairs of one row unit that the wave's half acts on; `pending`
// counts those since the wave's last fold.  At the end of a pair's body, before
// the barrier, the wave folds when the chain holds `cap` pairs (the most its
// integers stay exact for: Cfg::FOLD_PAIRS) or when the rows change behind
// this pair (peek()'s rows_change: another row unit, another slice of the same
// rows, or the walk's end) and the chain holds anything -- also in a wave that
// idles on this pair and acted on an earlier one of the unit.  The flush of
// the unit's sums stays behind the next barrier, after every wave's fold
// (tests/test_gram_fold_schedule.py walks this).
DAL_HD constexpr bool fold_due(int pending, int cap, bool rows_change) {
  return pending >= cap || (pending > 0 && rows_change);
}

// ---------------------------------------------------------------------------
// Host side: pair counts and the launch's grid and column chunks.

// Number of super blocks Q in [lo, hi) that super block I takes (O(1)): the
// closed form of sb_takes.
inline int64_t sb_pairs(int64_t I, int64_t lo, int64_t hi) {
  auto same_parity = [](int64_t a, int64_t b, int64_t p) -> int64_t {
    if (b <= a) return 0;
    return (b - p + 1) / 2 - (a - p + 1) / 2;
  };
  int64_t n = (lo <= I && I < hi) ? 1 : 0;
  n += same_parity(lo > I + 1 ? lo : I + 1, hi, I & 1);
  n += same_parity(lo, hi < I ? hi : I, (I & 1) ^ 1);
  return n;
}

// Pairs (P, J) for row super block P over 256-column blocks [a, b).
inline int64_t pairs_range(int64_t P, int64_t a, int64_t b) {
  if (b <= a) return 0;
  const int64_t qa = a >> 1, qb = (b - 1) >> 1;
  int64_t n = 2 * sb_pairs(P, qa, qb + 1);
  if ((a & 1) && sb_takes(P, qa)) --n;
  if (!((b - 1) & 1) && sb_takes(P, qb)) --n;
  return n;
}
inline int64_t pairs_skip(int64_t P, int64_t a, int64_t b, int64_t skip_lo, int64_t skip_hi) {
  const int64_t sa = a > skip_lo ? a : skip_lo, sb = b < skip_hi ? b : skip_hi;
  return pairs_range(P, a, b) - pairs_range(P, sa, sb);
}

// The chunk form's columns per chunk and chunk count for a requested count nc:
// equal chunks of ceil(nj / nc) columns, the last one short, none empty.
inline void column_chunks(int64_t nj, int64_t nc, int64_t* chunk_j, int64_t* n_chunks) {
  *chunk_j = (nj + nc - 1) / nc;
  *n_chunks = (nj + *chunk_j - 1) / *chunk_j;
}

// The most pairs any block of a G0-block grid multiplies with nc requested
// column chunks (a two-super-block unit costs the pairs of the busier one:
// they take the same column blocks but near the diagonal; so of four).
template <int HV>
int64_t chunked_max_load(int64_t srow0, int64_t n_srb, int64_t lo, int64_t hi, int64_t skip_lo, int64_t skip_hi,
                         int64_t ns_active, int64_t G0, int64_t nc, int64_t* n_chunks) {
  int64_t cbk;
  column_chunks(hi - lo, nc, &cbk, n_chunks);
  auto sched = [&](int64_t G, int64_t g) {
    return GramSchedule<HV>(static_cast<int>(srow0), static_cast<int>(n_srb), static_cast<int>(lo),
                            static_cast<int>(hi), static_cast<int>(skip_lo), static_cast<int>(skip_hi),
                            static_cast<int>(ns_active), static_cast<int>(cbk), static_cast<int>(*n_chunks), 0,
                            static_cast<int>(G), static_cast<int>(g));
  };
  const int64_t units = sched(1, 0).n_units(), G = units < G0 ? units : G0;
  int64_t mx = 0;
  for (int64_t g = 0; g < G; ++g) {
    const GramSchedule<HV> s = sched(G, g);
    int64_t load = 0;
    for (int u = s.first_seg(); u < s.n_seg; u += s.seg_step()) {
      int64_t w = 0;
      for (int h = 0; h < HV; ++h) {
        const int P = s.rowP(s.seg_ru(u), h);
        if (!s.live(P)) continue;
        const int64_t pw = pairs_skip(P, lo + s.seg_rlo(u), lo + s.seg_rhi(u), skip_lo, skip_hi);
        w = pw > w ? pw : w;
      }
      load += w;
    }
    mx = load > mx ? load : mx;
  }
  return mx;
}

// Column-chunk count for the round-robin units: the fewest chunks, at least
// kMinChunks, whose most loaded block has at most 8 % more pairs than the best
// balance found (exact pair counts; cached per shape).  More chunks = a
// smaller column working set swept by every block together (MALL hits; 2M x
// 256: 16 chunks 3.9 % faster than 1; 4 and 8: 0.6 % slower), fewer = fewer A
// loads and row flushes.  hv = super blocks per row unit (GramSchedule<hv>).
inline int64_t choose_chunks(int64_t srow0, int64_t n_srb, int64_t lo, int64_t hi, int64_t skip_lo, int64_t skip_hi,
                             int64_t ns_active, int64_t G0, int hv, int64_t kMinChunks) {
  struct Entry {
    int64_t k[10];
    int64_t nc;
  };
  static thread_local Entry cache[8] = {};
  static thread_local int cache_next = 0;
  const int64_t key[10] = {srow0, n_srb, lo, hi, skip_lo, skip_hi, ns_active, G0, hv, kMinChunks};
  for (const Entry& e : cache) {
    bool hit = e.nc > 0;
    for (int i = 0; i < 10 && hit; ++i) hit = e.k[i] == key[i];
    if (hit) return e.nc;
  }
  const int64_t nj = hi - lo;
  int64_t best_max = -1;
  std::vector<std::pair<int64_t, int64_t>> cand;
  int tried = 0;
  // chunk counts from 1 up (from kMinChunks when it is above 16 and the columns allow)
  for (int64_t c = kMinChunks > 16 && nj >= kMinChunks ? kMinChunks : 1; c <= nj && tried < 32; ++c) {
    if (c > 1 && (nj + c - 1) / c == (nj + c - 2) / (c - 1)) continue;  // the same chunks as c - 1
    ++tried;
    int64_t ncc;
    const int64_t mx = hv == 1   ? chunked_max_load<1>(srow0, n_srb, lo, hi, skip_lo, skip_hi, ns_active, G0, c, &ncc)
                       : hv == 2 ? chunked_max_load<2>(srow0, n_srb, lo, hi, skip_lo, skip_hi, ns_active, G0, c, &ncc)
                                 : chunked_max_load<4>(srow0, n_srb, lo, hi, skip_lo, skip_hi, ns_active, G0, c, &ncc);
    cand.emplace_back(ncc, mx);
    if (best_max < 0 || mx < best_max) best_max = mx;
  }
  int64_t best_nc = -1;
  for (int pass = 0; pass < 2 && best_nc < 0; ++pass)
    for (const auto& c : cand)
      if ((pass || c.first >= kMinChunks) && c.second * 100 <= best_max * 108) {
        best_nc = c.first;
        break;
      }
  if (best_nc < 0) best_nc = cand.back().first;
  Entry& e = cache[cache_next];
  cache_next = (cache_next + 1) % 8;
  for (int i = 0; i < 10; ++i) e.k[i] = key[i];
  e.nc = best_nc;
  return best_nc;
}

// The launch: its column chunks (chunk form: choose_chunks with at least
// min_chunks) and its grid -- the G0 blocks the device holds, or fewer when
// there are fewer pairs (contig) or units (chunk, over the launch's n_slices
// feature slices) to deal.  G == 0: no work.
struct GramLaunch {
  int chunk_j, n_chunks, G;
  int units;  // chunk form: the launch's units over its slices (contig: 0)
};
template <int HV>
GramLaunch plan_launch(int64_t srow0, int64_t n_srb, int64_t j_lo, int64_t j_hi, int64_t skip_lo, int64_t skip_hi,
                       int64_t ns_active, int64_t G0, int contig, int64_t min_chunks, int64_t n_slices = 1) {
  int64_t cbk = j_hi - j_lo, n_chunks = 1;
  if (!contig)
    column_chunks(j_hi - j_lo,
                  choose_chunks(srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi, ns_active, G0, HV, min_chunks), &cbk,
                  &n_chunks);
  const GramSchedule<HV> s(static_cast<int>(srow0), static_cast<int>(n_srb), static_cast<int>(j_lo),
                           static_cast<int>(j_hi), static_cast<int>(skip_lo), static_cast<int>(skip_hi),
                           static_cast<int>(ns_active), static_cast<int>(cbk), static_cast<int>(n_chunks), contig);
  const int64_t work = contig ? s.raw() : s.n_units() * n_slices;
  return {static_cast<int>(cbk), static_cast<int>(n_chunks), static_cast<int>(work < G0 ? (work > 0 ? work : 0) : G0),
          contig ? 0 : static_cast<int>(work)};
}

}  // namespace dal
