// Host driver of csrc/scaler_exact.hpp for tests/test_scaler_host.py: the fp32
// decomposition and the format rule are plain C++, so the code the kernels run
// is run here under AddressSanitizer and UBSan and compared with Python
// integers.
//
// Commands on stdin, answers on stdout (decimal):
//   V Q K1 K2 n    then n lines "<fp32 bits, hex>": per value
//                  "F <finite 0/1> <low> <top>" (low = top = 0 for a zero or a
//                  non-finite value), "L limb_0 .. limb_{K1-1}" of x at the
//                  quantum 2^Q and "S limb_0 .. limb_{K2-1}" of x*x at 2^(2Q)
//                  (both lines only for finite values); then the cells after
//                  adding every finite value "C word_0 .. word_{K1+K2-1}"
//   R d            then d lines "<low> <top>": "K <bad column> <k1> <k2>" and
//                  "Q q_0 .. q_{d-1}" (k1, k2, q only when bad column is -1)
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "scaler_exact.hpp"

namespace ex = dal::exact;
namespace sc = dal::scaler;

int main() {
  char cmd;
  while (scanf(" %c", &cmd) == 1) {
    if (cmd == 'V') {
      int Q, K1, K2, n;
      if (scanf("%d %d %d %d", &Q, &K1, &K2, &n) != 4) return 2;
      if (K1 < 1 || K1 > ex::kMaxLimbs || K2 < 1 || K2 > ex::kMaxLimbs || n < 0) return 2;
      std::vector<int64_t> cell(K1 + K2, 0);
      for (int i = 0; i < n; ++i) {
        uint32_t b;
        if (scanf("%" SCNx32, &b) != 1) return 2;
        const bool fin = sc::finite_f32(b);
        const ex::Parts p = sc::parts_f32(b);
        const bool nz = fin && p.mant != 0;
        printf("F %d %d %d\n", fin ? 1 : 0, nz ? sc::low_exponent(p) : 0, nz ? sc::top_exponent(p) : 0);
        if (!fin) continue;
        const ex::Parts s = sc::square(p);
        printf("L");
        for (int j = 0; j < K1; ++j) {
          const int32_t l = ex::limb(p, Q, j);
          printf(" %d", l);
          cell[j] += l;
        }
        printf("\nS");
        for (int j = 0; j < K2; ++j) {
          const int32_t l = ex::limb(s, 2 * Q, j);
          printf(" %d", l);
          cell[K1 + j] += l;
        }
        printf("\n");
      }
      printf("C");
      for (int64_t w : cell) printf(" %" PRId64, w);
      printf("\n");
    } else if (cmd == 'R') {
      int d;
      if (scanf("%d", &d) != 1 || d < 1) return 2;
      std::vector<int32_t> low(d), top(d), q(d, 0);
      for (int c = 0; c < d; ++c)
        if (scanf("%" SCNd32 " %" SCNd32, &low[c], &top[c]) != 2) return 2;
      int32_t k1 = 0, k2 = 0;
      const int64_t bad = sc::limb_counts(low.data(), top.data(), d, &k1, &k2, q.data());
      printf("K %" PRId64 " %d %d\nQ", bad, k1, k2);
      for (int c = 0; c < d; ++c) printf(" %d", q[c]);
      printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
