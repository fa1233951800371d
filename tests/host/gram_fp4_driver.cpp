// Host driver of tests/test_gram_fp4_algebra.py: csrc/gram_fp4.hpp's quantiser,
// 4-bit code and (h, l) -> (h', l') map on the values read from stdin (no HIP).
//   gram_fp4_driver         lines "h l"  ->  lines "a4 code decode(code) h' l'"  (%.17g)
//   gram_fp4_driver consts  ->  "kFp4AccShift kFp4Max kFp4ChainMax kFp4RowMax"
// "nan" is read as a NaN.
#include <cstdio>
#include <cstring>

#include "gram_fp4.hpp"

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "consts")) {
    std::printf("%d %d %d %d\n", dal::kFp4AccShift, dal::kFp4Max, dal::kFp4ChainMax, dal::kFp4RowMax);
    return 0;
  }
  double h, l;
  while (std::scanf("%lf %lf", &h, &l) == 2) {
    const int a = dal::quant_fp4(static_cast<float>(h));
    const unsigned code = dal::code_fp4(a);
    dal::requant_fp4(h, l);
    std::printf("%d %u %d %.17g %.17g\n", a, code, dal::decode_fp4(code), h, l);
  }
  return 0;
}
