// Host driver of csrc/rf_exact_sum.hpp for tests/test_rf_regress_host.py: the
// accumulator is plain C++, so the code the kernels run is run here under
// AddressSanitizer and UBSan and compared with Python integers.
//
// Commands on stdin, answers on stdout (decimal words, hex fp64 bits):
//   S Q K n        then n lines "<fp64 bits, hex> <weight>":
//                  per value "L limb_0 .. limb_{K-1}", then the cell after
//                  adding weight * limb in the given order "C word_0 ..", the
//                  same cell accumulated in reverse order "R word_0 ..", and
//                  "D <bits of to_double(cell)>"
//   O Q K          then two lines of K words (cells a, b):
//                  "A words of a + b", "B words of a - b",
//                  "D <bits of to_double(a + b)> <bits of to_double(a - b)>"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rf_exact_sum.hpp"

namespace ex = dal::exact;

static uint64_t bits_of(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}

static void print_words(const char* tag, const std::vector<int64_t>& c) {
  printf("%s", tag);
  for (int64_t w : c) printf(" %" PRId64, w);
  printf("\n");
}

static double cell_to_double(const std::vector<int64_t>& c, int Q) {
  const int64_t* p = c.data();
  return ex::to_double([p](int j) { return p[j]; }, static_cast<int>(c.size()), Q);
}

int main() {
  char cmd;
  int Q, K;
  while (scanf(" %c %d %d", &cmd, &Q, &K) == 3) {
    if (K < 1 || K > ex::kMaxLimbs) return 2;
    if (cmd == 'S') {
      int n;
      if (scanf("%d", &n) != 1 || n < 0) return 2;
      std::vector<double> y(n);
      std::vector<int64_t> w(n);
      for (int i = 0; i < n; ++i) {
        uint64_t b;
        if (scanf("%" SCNx64 " %" SCNd64, &b, &w[i]) != 2) return 2;
        memcpy(&y[i], &b, 8);
      }
      std::vector<int64_t> fwd(K, 0), rev(K, 0);
      for (int i = 0; i < n; ++i) {
        printf("L");
        for (int j = 0; j < K; ++j) {
          const int32_t l = ex::limb(y[i], Q, j);
          printf(" %d", l);
          fwd[j] += w[i] * l;
        }
        printf("\n");
      }
      for (int i = n - 1; i >= 0; --i)
        for (int j = 0; j < K; ++j) rev[j] += w[i] * ex::limb(y[i], Q, j);
      print_words("C", fwd);
      print_words("R", rev);
      printf("D %016" PRIx64 "\n", bits_of(cell_to_double(fwd, Q)));
    } else if (cmd == 'O') {
      std::vector<int64_t> a(K), b(K), s(K), d(K);
      for (int j = 0; j < K; ++j)
        if (scanf("%" SCNd64, &a[j]) != 1) return 2;
      for (int j = 0; j < K; ++j)
        if (scanf("%" SCNd64, &b[j]) != 1) return 2;
      ex::add(s.data(), 1, a.data(), 1, b.data(), 1, K);
      ex::sub(d.data(), 1, a.data(), 1, b.data(), 1, K);
      print_words("A", s);
      print_words("B", d);
      printf("D %016" PRIx64 " %016" PRIx64 "\n", bits_of(cell_to_double(s, Q)), bits_of(cell_to_double(d, Q)));
    } else {
      return 2;
    }
  }
  return 0;
}
