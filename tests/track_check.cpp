// Stand-alone host check of csrc/track_sizes.h (no GPU, no HIP): every refusal of a
// tracking spec at its boundary values and in the order of the checks, the byte size of
// the reference with its 32-bit-offset bound at the last accepted and first refused
// value, the bytes of cost_agent, the row clamp at both ends of int32, and the fold's
// grid.  Built and run by tests/test_track_host.py with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "track_sizes.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace qs;
  CHECK(kTrackState == 12 && kTrackMaxAct == 4 && kTrackRowBytes == 48 && kTrackAlign == 16);

  // ---- a weight: finite and >= 0; -0.0 is 0; negatives, NaN and the infinities are out
  const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
  const float tiny = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
  for (float w : {0.0f, -0.0f, tiny, 1.0f, 2.5f, big}) CHECK(track_weight_ok(w));
  for (float w : {-tiny, -1.0f, -big, inf, -inf, nan, -nan}) CHECK(!track_weight_ok(w));

  // ---- refusals, in the order of the checks.  E = 21, D = 8, A = 1
  TrackSpecShape ok{};
  ok.ref = 0x1000;
  ok.L = 3;
  for (float& q : ok.q) q = 1.0f;
  for (float& r : ok.r) r = 0.5f;
  ok.terminal = 2.5f;
  ok.reward_scale = -1.0f;
  CHECK(track_refusal(ok, 21, 8, 1) == kTrackOk);
  TrackSpecShape v = ok;
  v.ref = 0; CHECK(track_refusal(v, 21, 8, 1) == kTrackRefNull);
  for (uintptr_t off : {1u, 4u, 8u, 12u, 15u}) { v = ok; v.ref = 0x1000 + off; CHECK(track_refusal(v, 21, 8, 1) == kTrackRefAlign); }
  for (uintptr_t off : {16u, 32u, 256u}) { v = ok; v.ref = 0x1000 + off; CHECK(track_refusal(v, 21, 8, 1) == kTrackOk); }
  for (int64_t L : {(int64_t)0, (int64_t)-1, (int64_t)std::numeric_limits<int32_t>::min()}) {
    v = ok; v.L = L; CHECK(track_refusal(v, 21, 8, 1) == kTrackRows);
  }
  v = ok; v.L = 1; CHECK(track_refusal(v, 21, 8, 1) == kTrackOk);
  for (int k = 0; k < kTrackState; ++k) {
    for (float w : {-tiny, -1.0f, nan, inf}) { v = ok; v.q[k] = w; CHECK(track_refusal(v, 21, 8, 1) == kTrackQ); }
    for (float w : {0.0f, -0.0f, big}) { v = ok; v.q[k] = w; CHECK(track_refusal(v, 21, 8, 1) == kTrackOk); }
  }
  for (int A = 1; A <= 4; ++A)
    for (int a = 0; a < kTrackMaxAct; ++a)
      for (float w : {-tiny, nan, inf}) {   // components from A on are not read
        v = ok; v.r[a] = w; CHECK(track_refusal(v, 21, 8, A) == (a < A ? kTrackR : kTrackOk));
      }
  for (float w : {-tiny, -2.5f, nan, inf, -inf}) { v = ok; v.terminal = w; CHECK(track_refusal(v, 21, 8, 1) == kTrackTerminal); }
  for (float w : {0.0f, -0.0f, big}) { v = ok; v.terminal = w; CHECK(track_refusal(v, 21, 8, 1) == kTrackOk); }
  for (float w : {nan, inf, -inf}) { v = ok; v.reward_scale = w; CHECK(track_refusal(v, 21, 8, 1) == kTrackScale); }
  for (float w : {0.0f, -0.0f, -big, big}) { v = ok; v.reward_scale = w; CHECK(track_refusal(v, 21, 8, 1) == kTrackOk); }
  // the order: an earlier refusal wins
  v = ok; v.ref = 0; v.L = 0; v.q[0] = nan; CHECK(track_refusal(v, 21, 8, 1) == kTrackRefNull);
  v = ok; v.ref = 0x1004; v.L = 0; CHECK(track_refusal(v, 21, 8, 1) == kTrackRefAlign);
  v = ok; v.L = 0; v.q[3] = -1.0f; CHECK(track_refusal(v, 21, 8, 1) == kTrackRows);
  v = ok; v.q[11] = nan; v.r[0] = nan; CHECK(track_refusal(v, 21, 8, 1) == kTrackQ);
  v = ok; v.r[0] = nan; v.terminal = nan; CHECK(track_refusal(v, 21, 8, 1) == kTrackR);
  v = ok; v.terminal = nan; v.reward_scale = nan; CHECK(track_refusal(v, 21, 8, 1) == kTrackTerminal);
  v = ok; v.reward_scale = nan; v.L = int64_t(1) << 40; CHECK(track_refusal(v, 21, 8, 1) == kTrackScale);

  // ---- the reference's bytes and the 32-bit bound: L · E · D · 48 < 2^31
  uint64_t b = 0;
  CHECK(track_ref_bytes(3, 21, 8, &b) && b == 3u * 21u * 8u * 48u);
  CHECK(track_ref_bytes(1, 1, 1, &b) && b == 48u);
  const uint64_t lim = uint64_t(1) << 31;
  {
    const int64_t E = 21, D = 8, last = (int64_t)((lim - 1) / (uint64_t)(E * D * 48));
    CHECK((uint64_t)(last * E * D * 48) < lim && (uint64_t)((last + 1) * E * D * 48) >= lim);
    CHECK(track_ref_bytes(last, E, D, &b) && b == (uint64_t)(last * E * D * 48));
    b = 7; CHECK(!track_ref_bytes(last + 1, E, D, &b) && b == 7);
    v = ok; v.L = last; CHECK(track_refusal(v, E, D, 1) == kTrackOk);
    v = ok; v.L = last + 1; CHECK(track_refusal(v, E, D, 1) == kTrackOffsets);
  }
  {   // large rows
    const int64_t E = int64_t(1) << 20, D = 16;   // a row is 2^24 · 48 bytes = 3 · 2^28
    CHECK(track_ref_bytes(2, E, D, &b) && b == uint64_t(3) << 29);   // 1.5 · 2^30 < 2^31
    CHECK(!track_ref_bytes(3, E, D, &b));                            // 2.25 · 2^30 >= 2^31
  }
  // empty and oversized axes, products that would wrap 64 bits
  const int64_t i32max = std::numeric_limits<int32_t>::max(), i64max = std::numeric_limits<int64_t>::max();
  for (int64_t bad : {(int64_t)0, (int64_t)-1, i64max, int64_t(1) << 31}) {
    CHECK(!track_ref_bytes(bad, 1, 1, &b));
    CHECK(!track_ref_bytes(1, bad, 1, &b));
    CHECK(!track_ref_bytes(1, 1, bad, &b));
  }
  CHECK(!track_ref_bytes(i32max, i32max, i32max, &b));
  CHECK(!track_ref_bytes(i32max, i32max, 1, &b) && !track_ref_bytes(i32max, 1, i32max, &b));
  CHECK(track_ref_bytes((int64_t)((lim - 1) / 48), 1, 1, &b) && b == (lim - 1) / 48 * 48);
  CHECK(!track_ref_bytes((int64_t)((lim - 1) / 48) + 1, 1, 1, &b));

  // ---- cost_agent
  CHECK(track_cost_bytes(3, 21, 8) == 3u * 21u * 8u * 8u);
  CHECK(track_cost_bytes(4096, 16, 8) == uint64_t(4096) * 16 * 8 * 8);

  // ---- the row a step reads: clamp(base + j, 0, L − 1) without a sum that wraps
  const int32_t imin = std::numeric_limits<int32_t>::min(), imax = std::numeric_limits<int32_t>::max();
  CHECK(track_row(0, 0, 3) == 0 && track_row(0, 1, 3) == 1 && track_row(0, 2, 3) == 2 && track_row(0, 3, 3) == 2);
  CHECK(track_row(-2, 0, 3) == 0 && track_row(-2, 2, 3) == 0 && track_row(-2, 3, 3) == 1 && track_row(-2, 31, 3) == 2);
  CHECK(track_row(2, 0, 3) == 2 && track_row(3, 0, 3) == 2 && track_row(7, 31, 3) == 2);
  CHECK(track_row(imax, 31, 3) == 2 && track_row(imax, 0, imax) == imax - 1 && track_row(imax - 1, 31, imax) == imax - 1);
  CHECK(track_row(imin, 0, 3) == 0 && track_row(imin, 31, 3) == 0 && track_row(-31, 31, 3) == 0 && track_row(-31, 30, 1) == 0);
  for (int32_t j = 0; j < 32; ++j) CHECK(track_row(5, j, 1) == 0 && track_row(-5, j, 1) == 0);
  // the kernel's form of the same value: a base at or past L never has j added (L is at
  // most (2^31 − 1) / 48 there, so base + j cannot wrap below it)
  const int32_t Lmax = (int32_t)((lim - 1) / 48);
  for (int32_t base : {imin, -40, -2, -1, 0, 1, 2, 3, 4, 40, Lmax - 2, Lmax - 1, Lmax, imax - 1, imax})
    for (int32_t L : {1, 2, 3, 17, Lmax})
      for (int32_t j : {0, 1, 5, 31}) {
        int32_t row = base >= L ? L - 1 : base + j;
        row = row < 0 ? 0 : (row > L - 1 ? L - 1 : row);
        CHECK(row == track_row(base, j, L));
      }

  // ---- the fold's grid: one thread per (c, e), kTrackFoldThreads a workgroup
  CHECK(kTrackFoldThreads == 256);
  CHECK(track_fold_grid(1, 1) == 1 && track_fold_grid(16, 16) == 1 && track_fold_grid(257, 1) == 2);
  CHECK(track_fold_grid(4096, 1) == 16 && track_fold_grid(256, 64) == 64 && track_fold_grid(4, 4096) == 64);
  CHECK(track_fold_grid(3, 21) == 1 && track_fold_grid(2, 700) == 6);
  CHECK(track_fold_grid(0, 5) == 0 && track_fold_grid(5, 0) == 0 && track_fold_grid(-1, 5) == 0);
  CHECK(track_fold_grid(int64_t(1) << 31, 1) == 0 && track_fold_grid(1 << 16, 1 << 15) == 0);
  CHECK(track_fold_grid(1 << 16, (1 << 15) - 1) == (uint32_t)((((uint64_t)1 << 16) * ((1 << 15) - 1) + 255) / 256));
  CHECK(track_fold_grid(i64max, i64max) == 0);

  std::printf("track_sizes ok\n");
  return 0;
}
