// Host driver of csrc/sq_error_exact.hpp (over csrc/rf_exact_sum.hpp) for
// tests/test_metrics_host.py: the squared error, its format rule and its limbs
// are plain C++, so the code the kernels run is run here under
// AddressSanitizer and UBSan and compared with Python integers.
//
// Commands on stdin, answers on stdout (decimal words, hex fp64 bits):
//   F n            then n lines "<pred bits, hex> <y bits, hex>":
//                  per row "S <bits of s> <finite 0/1> <low> <top>" (low and
//                  top 0 for a zero or non-finite s), then
//                  "M <min low> <max top> <any non-finite 0/1>" (INT32_MAX /
//                  INT32_MIN when no s is nonzero)
//   A Q K n        then n lines as above: per row "L limb_0 .. limb_{K-1}" of
//                  s for the quantum 2^Q, then the cell "C word_0 .. word_{K-1}"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sq_error_exact.hpp"

namespace ex = dal::exact;
namespace sq = dal::sqerr;

static uint64_t bits_of(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}

static bool read_rows(int n, std::vector<double>& s) {
  s.resize(n);
  for (int i = 0; i < n; ++i) {
    uint64_t pb, yb;
    if (scanf("%" SCNx64 " %" SCNx64, &pb, &yb) != 2) return false;
    double p, y;
    memcpy(&p, &pb, 8);
    memcpy(&y, &yb, 8);
    s[i] = sq::squared_error(p, y);
  }
  return true;
}

int main() {
  char cmd;
  while (scanf(" %c", &cmd) == 1) {
    std::vector<double> s;
    if (cmd == 'F') {
      int n;
      if (scanf("%d", &n) != 1 || n < 0 || !read_rows(n, s)) return 2;
      int32_t low = sq::kNoLow, top = sq::kNoTop;
      int bad = 0;
      for (int i = 0; i < n; ++i) {
        const bool fin = sq::finite_f64(s[i]);
        int lo = 0, hi = 0;
        if (!fin) {
          bad = 1;
        } else {
          const ex::Parts p = ex::parts(s[i]);
          if (p.mant) {
            lo = sq::low_exponent(p);
            hi = sq::top_exponent(p);
            if (lo < low) low = lo;
            if (hi > top) top = hi;
          }
        }
        printf("S %016" PRIx64 " %d %d %d\n", bits_of(s[i]), fin ? 1 : 0, lo, hi);
      }
      printf("M %d %d %d\n", low, top, bad);
    } else if (cmd == 'A') {
      int Q, K, n;
      if (scanf("%d %d %d", &Q, &K, &n) != 3 || K < 1 || K > ex::kMaxLimbs || n < 0 || !read_rows(n, s)) return 2;
      std::vector<int64_t> cell(K, 0);
      for (int i = 0; i < n; ++i) {
        printf("L");
        for (int j = 0; j < K; ++j) {
          const int32_t l = ex::limb(s[i], Q, j);
          printf(" %d", l);
          cell[j] += l;
        }
        printf("\n");
      }
      printf("C");
      for (int64_t w : cell) printf(" %" PRId64, w);
      printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
