// Host driver of tests/test_gram_i8_algebra.py: csrc/gram_i8.hpp's quantiser
// and (h, l) -> (h', l') map on the values read from stdin (no HIP).
//   gram_i8_driver          lines "h l"  ->  lines "a h' l'"  (%.17g)
#include <cstdio>

#include "gram_i8.hpp"

int main() {
  double h, l;
  while (std::scanf("%lf %lf", &h, &l) == 2) {
    const int a = dal::quant_i8(static_cast<float>(h));
    dal::requant_i8(h, l);
    std::printf("%d %.17g %.17g\n", a, h, l);
  }
  return 0;
}
