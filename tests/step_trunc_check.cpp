// Stand-alone host check of csrc/step_trunc.h (no GPU, no HIP): the integer
// truncation threshold against the division form it replaces.  Built and run by
// tests/test_step_trunc_host.py with -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "step_trunc.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  const int freqs[] = {240, 48, 30, 1000, 7};
  const double secs[] = {0.0, 8.0, 12.0, 1.0 / 3.0, 0.1, 8.0 + std::ldexp(1.0, -40), 1e7};
  for (int f : freqs) {
    for (double L : secs) {
      const int64_t n = qs::trunc_threshold_exact(f, L);   // n*, before the int32 clamp
      const int32_t at = qs::trunc_threshold(f, L);        // what the kernel compares against
      CHECK(n >= 0 && n != qs::kTruncNever);
      CHECK(at == (n > INT32_MAX ? INT32_MAX : (int32_t)n));
      // n* satisfies the predicate and n* − 1 does not
      CHECK(qs::trunc_by_division(n, f, L));
      if (n > 0) CHECK(!qs::trunc_by_division(n - 1, f, L));
      // the kernel's test equals the division form for every counter around n*
      const int64_t lo = n - 1000 < 0 ? 0 : n - 1000;
      const int64_t hi = n + 1000 > INT32_MAX ? INT32_MAX : n + 1000;
      for (int64_t c = lo; c <= hi; ++c) CHECK(((int32_t)c >= at) == qs::trunc_by_division(c, f, L));
    }
  }
  // known values: 8 s at 240 Hz is passed by counter 1921; 0 s by counter 1
  CHECK(qs::trunc_threshold(240, 8.0) == 1921);
  CHECK(qs::trunc_threshold(240, 0.0) == 1);
  CHECK(qs::trunc_threshold(240, -1.0) == 0);
  // the clamp: 1e7 s at 1000 Hz needs counter 1e10 + 1, which no int32 counter reaches
  CHECK(qs::trunc_threshold_exact(1000, 1e7) == 10000000001LL);
  CHECK(qs::trunc_threshold(1000, 1e7) == INT32_MAX);
  CHECK(!qs::trunc_by_division(INT32_MAX - 1, 1000, 1e7));
  // no counter at all: NaN, infinity
  CHECK(qs::trunc_threshold(240, std::nan("")) == INT32_MAX);
  CHECK(qs::trunc_threshold(240, INFINITY) == INT32_MAX);
  std::printf("step_trunc ok\n");
  return 0;
}
