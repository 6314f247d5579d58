// Stand-alone host check of csrc/avoid_sizes.h (no GPU, no HIP): every refusal of an
// avoidance spec at its boundary values and in the order of the checks, the table's bytes,
// the two switches, and the overlap test of cost_agent at touching and crossing ranges.
// Built and run by tests/test_avoid_host.py with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "avoid_sizes.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace qs;
  CHECK(kAvoidMaxRows == 16 && kAvoidRowFloats == 8 && kAvoidRowBytes == 32 && kAvoidAlign == 16);

  // ---- a radius, weight or scale: finite and >= 0; -0.0 is 0; negatives, NaN and the infinities are out
  const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
  const float tiny = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
  for (float w : {0.0f, -0.0f, tiny, 1.0f, 2.5f, big}) CHECK(avoid_number_ok(w));
  for (float w : {-tiny, -1.0f, -big, inf, -inf, nan, -nan}) CHECK(!avoid_number_ok(w));

  // ---- refusals, in the order of the checks
  const AvoidSpecShape ok{0x1000, 4, 1.2f, 0.7f, 0.5f};
  CHECK(avoid_refusal(ok) == kAvoidOk && avoid_refusal_text(kAvoidOk) == nullptr);
  AvoidSpecShape v = ok;
  for (int64_t M : {(int64_t)-1, (int64_t)17, (int64_t)std::numeric_limits<int32_t>::min(),
                    (int64_t)std::numeric_limits<int32_t>::max()}) {
    v = ok; v.M = M; CHECK(avoid_refusal(v) == kAvoidRows);
  }
  for (int64_t M : {(int64_t)1, (int64_t)15, (int64_t)16}) { v = ok; v.M = M; CHECK(avoid_refusal(v) == kAvoidOk); }
  v = ok; v.obstacles = 0; CHECK(avoid_refusal(v) == kAvoidTabNull);
  for (uintptr_t off : {1u, 4u, 8u, 12u, 15u}) { v = ok; v.obstacles = 0x1000 + off; CHECK(avoid_refusal(v) == kAvoidTabAlign); }
  for (uintptr_t off : {16u, 32u, 256u}) { v = ok; v.obstacles = 0x1000 + off; CHECK(avoid_refusal(v) == kAvoidOk); }
  // M == 0 reads no table: a null or misaligned pointer is fine
  for (uintptr_t p : {(uintptr_t)0, (uintptr_t)0x1004, (uintptr_t)1}) { v = ok; v.M = 0; v.obstacles = p; CHECK(avoid_refusal(v) == kAvoidOk); }
  // ... but the row count is checked first
  v = ok; v.M = 17; v.obstacles = 0; CHECK(avoid_refusal(v) == kAvoidRows);
  for (float w : {-tiny, -1.0f, nan, inf, -inf}) {
    v = ok; v.sep_radius = w; CHECK(avoid_refusal(v) == kAvoidRadius);
    v = ok; v.sep_weight = w; CHECK(avoid_refusal(v) == kAvoidWeight);
    v = ok; v.sep_z_scale = w; CHECK(avoid_refusal(v) == kAvoidZScale);
  }
  for (float w : {0.0f, -0.0f, tiny, big}) {
    v = ok; v.sep_radius = w; CHECK(avoid_refusal(v) == kAvoidOk);
    v = ok; v.sep_weight = w; CHECK(avoid_refusal(v) == kAvoidOk);
    v = ok; v.sep_z_scale = w; CHECK(avoid_refusal(v) == kAvoidOk);
  }
  // the order: rows, table, radius, weight, scale
  v = ok; v.obstacles = 4; v.sep_radius = nan; v.sep_weight = nan; v.sep_z_scale = nan;
  CHECK(avoid_refusal(v) == kAvoidTabAlign);
  v.obstacles = 0x1000; CHECK(avoid_refusal(v) == kAvoidRadius);
  v.sep_radius = 1.0f; CHECK(avoid_refusal(v) == kAvoidWeight);
  v.sep_weight = 1.0f; CHECK(avoid_refusal(v) == kAvoidZScale);
  // every refusal has a text of its own
  const AvoidRefusal all[] = {kAvoidRows, kAvoidTabNull, kAvoidTabAlign, kAvoidRadius, kAvoidWeight, kAvoidZScale};
  for (AvoidRefusal a : all) {
    CHECK(avoid_refusal_text(a) != nullptr);
    for (AvoidRefusal b : all) CHECK(a == b || std::strcmp(avoid_refusal_text(a), avoid_refusal_text(b)) != 0);
  }

  // ---- the table's bytes
  CHECK(avoid_table_bytes(0) == 0 && avoid_table_bytes(1) == 32 && avoid_table_bytes(16) == 512);

  // ---- the switches: a term that is off is skipped
  CHECK(avoid_sep_on(1.2f, 0.7f, 2) && avoid_sep_on(tiny, tiny, 16));
  CHECK(!avoid_sep_on(0.0f, 0.7f, 8) && !avoid_sep_on(-0.0f, 0.7f, 8) && !avoid_sep_on(1.2f, 0.0f, 8) &&
        !avoid_sep_on(1.2f, -0.0f, 8) && !avoid_sep_on(1.2f, 0.7f, 1));
  CHECK(!avoid_obs_on(0) && avoid_obs_on(1) && avoid_obs_on(16));

  // ---- cost_agent against another range [0x2000, 0x3000): touching is not meeting
  CHECK(!avoid_ranges_meet(0x1000, 0x1000, 0x2000, 0x3000));   // ends where the other starts
  CHECK(avoid_ranges_meet(0x1000, 0x1001, 0x2000, 0x3000));    // one byte in
  CHECK(avoid_ranges_meet(0x2000, 8, 0x2000, 0x3000) && avoid_ranges_meet(0x2ff8, 8, 0x2000, 0x3000));
  CHECK(avoid_ranges_meet(0x2fff, 8, 0x2000, 0x3000));         // the last byte
  CHECK(!avoid_ranges_meet(0x3000, 8, 0x2000, 0x3000));        // starts where the other ends
  CHECK(avoid_ranges_meet(0x1000, 0x4000, 0x2000, 0x3000));    // round it

  std::printf("avoid_sizes ok\n");
  return 0;
}
