// Stand-alone host check of csrc/step_score.h (no GPU, no HIP): how many steps a
// branch-rollout launch (qs_score) takes, the byte sizes of its buffers over
// C · E virtual envs, and the overlap test over outputs and action buffers.
// Built and run by tests/test_step_score_host.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "step_score.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using qs::score_depth;
  // ---- depth.  The figures quadswarm.hip passes: 64 KB per workgroup, of which
  // 8 192 static + 512 grain are fixed; a history image is H · 64 · A · 4 bytes,
  // the obs stage rows · O · 4 bytes, a step's action rows 256 · A bytes.
  const size_t lim = 64 * 1024, fixed = 8192 + 512;
  CHECK(qs::kScoreMaxSteps == 32 && qs::kScoreStepBytes == 256);
  // A = 1, 30 Hz (history in registers): O = 12 + 15 = 27, 64 rows: 6 912 of stage.
  // 65 536 − 8 704 − 6 912 = 49 920 free = 195 rows: the cap
  CHECK(score_depth(lim, fixed, 0, 64 * 27 * 4, 1) == 32);
  // A = 1, 60 Hz (H = 30, image 7 680; O = 42, stage 10 752): 38 400 free = 150 rows
  CHECK(score_depth(lim, fixed, 30 * 64 * 1 * 4, 64 * 42 * 4, 1) == 32);
  // A = 3, 30 Hz: O = 57, stage 14 592: 42 240 free / 768 = 55
  CHECK(score_depth(lim, fixed, 0, 64 * 57 * 4, 3) == 32);
  // A = 3, 60 Hz: image 30 · 64 · 3 · 4 = 23 040, O = 102, stage 26 112: 7 680 free / 768 = 10
  CHECK(score_depth(lim, fixed, 23040, 26112, 3) == 10);
  // A = 4, 30 Hz in registers: O = 72, stage 18 432: 38 400 free / 1 024 = 37
  CHECK(score_depth(lim, fixed, 0, 64 * 72 * 4, 4) == 32);
  // A = 4 with the image (CF2P: run-time frequency; H = 15, image 15 360): 23 040 free / 1 024 = 22.5
  CHECK(score_depth(lim, fixed, 15 * 64 * 4 * 4, 64 * 72 * 4, 4) == 22);
  // whole rows only, and none at all
  CHECK(score_depth(lim, lim - 1024, 0, 0, 4) == 1);
  CHECK(score_depth(lim, lim - 1023, 0, 0, 4) == 0);
  CHECK(score_depth(lim, lim - 2047, 0, 0, 4) == 1);
  CHECK(score_depth(lim, lim - 2048, 0, 0, 4) == 2);
  CHECK(score_depth(lim, lim, 0, 0, 1) == 0);
  CHECK(score_depth(lim, lim, 16, 16, 1) == 0);          // past the limit: no wrap
  CHECK(score_depth(lim, 0, 0, 0, 0) == 0);              // no action width

  // ---- sizes: b[0..6] a step's outputs, b[7] ret, b[8] first_done
  uint64_t b[qs::kScoreOuts], act = 0;
  CHECK(qs::score_sizes(qs::ScoreShape{3, 21, 8, 27, 1, 4}, b, &act));
  CHECK(b[0] == 3u * 21 * 8 * 27 * 4 && b[1] == 3u * 21 * 4 && b[2] == 63 && b[3] == 63 && b[4] == b[0]);
  CHECK(b[5] == 3u * 21 * 8 && b[6] == 3u * 21 * 8 * 4 && b[7] == 63u * 8 && b[8] == 63u * 4 && act == b[6]);
  CHECK(qs::score_sizes(qs::ScoreShape{3, 21, 8, 27, 4, 8}, b, &act) && b[1] == 63u * 8 && act == 63u * 8 * 16);
  CHECK(!qs::score_sizes(qs::ScoreShape{0, 21, 8, 27, 1, 4}, b, &act));
  CHECK(!qs::score_sizes(qs::ScoreShape{-1, 21, 8, 27, 1, 4}, b, &act));
  // C · E · D · O · 4 around 2^31: C · E = 2^16, D = 8, O = 1024 is 2^31 bytes exactly
  CHECK(qs::score_sizes(qs::ScoreShape{1 << 8, 1 << 8, 8, 1024, 1, 4}, b, &act));
  CHECK(b[0] == (uint64_t(1) << 31) && !qs::score_fits(b[0]) && qs::score_fits(b[0] - 1) && qs::score_fits(b[6]));
  CHECK(qs::score_sizes(qs::ScoreShape{1 << 8, 1 << 8, 8, 1023, 1, 4}, b, &act) && qs::score_fits(b[0]));
  // obs elements near 2^31 (bytes near 2^33): sized without wrapping, refused by score_fits
  CHECK(qs::score_sizes(qs::ScoreShape{1 << 10, 1 << 10, 8, 255, 1, 4}, b, &act));
  CHECK(b[0] == uint64_t(1 << 20) * 8 * 255 * 4 && !qs::score_fits(b[0]) && qs::score_fits(b[1]));
  // the virtual agent count itself: 2^31 − 8 agents pass, 2^31 do not; nor does C · E = 2^31
  CHECK(qs::score_sizes(qs::ScoreShape{(1 << 28) - 1, 1, 8, 27, 1, 4}, b, &act) && !qs::score_fits(b[0]));
  CHECK(!qs::score_sizes(qs::ScoreShape{1 << 28, 1, 8, 27, 1, 4}, b, &act));
  CHECK(!qs::score_sizes(qs::ScoreShape{1 << 16, 1 << 15, 1, 27, 1, 4}, b, &act));
  CHECK(!qs::score_sizes(qs::ScoreShape{2147483647, 2147483647, 64, 27, 4, 8}, b, &act));

  // ---- overlap: outputs against outputs and against actions; actions may share
  std::vector<unsigned char> mem(4096);
  unsigned char* m = mem.data();
  auto R = [] { return qs::ScoreRanges(); };
  {   // adjacent ranges touch without overlapping, in any order of arrival
    qs::ScoreRanges r = R();
    CHECK(r.add(m + 64, 64, false) && r.add(m, 64, false) && r.add(m + 128, 32, true) && r.add(m + 160, 8, false));
    CHECK(r.n == 4 && !r.overlap());
  }
  {   // one byte into the next output
    qs::ScoreRanges r = R();
    r.add(m, 65, false); r.add(m + 64, 64, false);
    CHECK(r.overlap());
  }
  {   // nested: an output inside another output; inside an action buffer; an action buffer inside an output
    qs::ScoreRanges r = R();
    r.add(m, 256, false); r.add(m + 100, 4, false);
    CHECK(r.overlap());
    r = R();
    r.add(m, 256, true); r.add(m + 100, 4, false);
    CHECK(r.overlap());
    r = R();
    r.add(m, 256, false); r.add(m + 100, 4, true);
    CHECK(r.overlap());
    r = R();   // … and an output past a short action range that lies inside a long one
    r.add(m, 256, true); r.add(m + 8, 8, true); r.add(m + 200, 8, false);
    CHECK(r.overlap());
  }
  {   // equal ranges: two outputs, an output and an action buffer; two action buffers are fine
    qs::ScoreRanges r = R();
    r.add(m, 64, false); r.add(m, 64, false);
    CHECK(r.overlap());
    r = R();
    r.add(m, 64, true); r.add(m, 64, false);
    CHECK(r.overlap());
    r = R();
    r.add(m, 64, false); r.add(m, 64, true);
    CHECK(r.overlap());
    r = R();
    for (int j = 0; j < 32; ++j) r.add(m, 64, true);   // every step reads the same buffer
    r.add(m + 32, 64, true);
    r.add(m + 96, 16, false);
    CHECK(!r.overlap());
    r.add(m + 95, 1, false);
    CHECK(r.overlap());
  }
  {   // null pointers are no ranges; a full call's worth fits and one more does not
    qs::ScoreRanges r = R();
    CHECK(r.add(nullptr, 64, false) && r.add(nullptr, 64, true) && r.n == 0 && !r.overlap());
    for (int i = 0; i < qs::kScoreMaxRanges; ++i) CHECK(r.add(m + 8 * i, 8, i % 8 == 0));
    CHECK(r.n == qs::kScoreMaxRanges && !r.add(m + 4000, 8, false) && r.n == qs::kScoreMaxRanges);
    CHECK(!r.overlap());
  }
  std::printf("step_score ok\n");
  return 0;
}
