// Stand-alone host check of csrc/planner_sizes.h (no GPU, no HIP): the byte sizes
// of an MPPI planner's buffers with their overflow refusals, the choice between
// the two reduction variants at its boundaries, and the launch grids.
// Built and run by tests/test_mppi_host.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "planner_sizes.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace qs;
  uint64_t b[kMppiBufs];
  // ---- sizes.  n = 16, C = 4 096, E = 1, D = 8, A = 1 (the advertised scoring shape)
  CHECK(mppi_sizes(MppiShape{16, 4096, 1, 8, 1}, b));
  CHECK(b[kMppiNominal] == 16u * 8 * 4 && b[kMppiCandidates] == 16ull * 4096 * 8 * 4);
  CHECK(b[kMppiRet] == 4096u * 8 && b[kMppiFirstDone] == 4096u * 4 && b[kMppiWeights] == 4096u * 8);
  CHECK(b[kMppiBest] == 4 && b[kMppiAction] == 8 * 4 && b[kMppiTick] == 8);
  // A = 4, an odd env count
  CHECK(mppi_sizes(MppiShape{7, 3, 21, 3, 4}, b));
  CHECK(b[kMppiNominal] == 7u * 21 * 12 * 4 && b[kMppiCandidates] == 7u * 3 * 21 * 12 * 4);
  CHECK(b[kMppiRet] == 63u * 8 && b[kMppiFirstDone] == 63u * 4 && b[kMppiBest] == 21u * 4 && b[kMppiAction] == 21u * 48);
  // ---- refusals: horizon, candidates, components
  CHECK(!mppi_sizes(MppiShape{0, 4, 1, 8, 1}, b) && !mppi_sizes(MppiShape{33, 4, 1, 8, 1}, b));
  CHECK(mppi_sizes(MppiShape{1, 2, 1, 1, 1}, b) && mppi_sizes(MppiShape{32, 2, 1, 1, 1}, b));
  CHECK(!mppi_sizes(MppiShape{8, 1, 1, 8, 1}, b) && !mppi_sizes(MppiShape{8, 0, 1, 8, 1}, b) &&
        !mppi_sizes(MppiShape{8, -5, 1, 8, 1}, b));
  CHECK(!mppi_sizes(MppiShape{8, 4, 0, 8, 1}, b) && !mppi_sizes(MppiShape{8, 4, 1, 0, 1}, b) &&
        !mppi_sizes(MppiShape{8, 4, 1, 8, 0}, b) && !mppi_sizes(MppiShape{8, 4, 1, 8, 5}, b));
  // a row of D · A components: at most kMppiMaxRow = 256
  CHECK(mppi_sizes(MppiShape{8, 4, 1, 64, 4}, b) && !mppi_sizes(MppiShape{8, 4, 1, 65, 4}, b));
  CHECK(mppi_sizes(MppiShape{8, 4, 1, 256, 1}, b) && !mppi_sizes(MppiShape{8, 4, 1, 257, 1}, b));
  // the counter word c · 32 + j: at most 2^27 candidates (D = A = 1, E = 1: 2^27 · 4 B a step, fine otherwise)
  CHECK(mppi_sizes(MppiShape{32, int64_t(1) << 27, 1, 1, 1}, b));
  CHECK(b[kMppiCandidates] == (uint64_t(32) << 27) * 4u);   // 2^34 bytes: past 32 bits as a whole, each step within
  CHECK(!mppi_sizes(MppiShape{32, (int64_t(1) << 27) + 1, 1, 1, 1}, b));
  // qs_score's 32-bit offsets: C · E virtual envs, C · E · D virtual agents, a step's actions, ret
  CHECK(!mppi_sizes(MppiShape{8, 1 << 16, 1 << 15, 1, 1}, b));               // C · E = 2^31
  CHECK(mppi_sizes(MppiShape{8, 1 << 14, 1 << 13, 1, 1}, b));                // 2^27 virtual envs, 2^30 B of ret
  CHECK(!mppi_sizes(MppiShape{8, 1 << 14, 1 << 14, 1, 1}, b));               // ret: 2^28 · 8 = 2^31 B
  CHECK(!mppi_sizes(MppiShape{8, 1 << 12, 1 << 12, 128, 1}, b));             // C · E · D = 2^31
  CHECK(mppi_sizes(MppiShape{8, 1 << 12, 1 << 12, 31, 1}, b));               // a step: 2^24 · 31 · 4 < 2^31 B
  CHECK(!mppi_sizes(MppiShape{8, 1 << 12, 1 << 12, 32, 1}, b));              // a step: 2^31 B
  CHECK(!mppi_sizes(MppiShape{8, 1 << 12, 1 << 12, 8, 4}, b));               // the same through A
  CHECK(!mppi_sizes(MppiShape{8, 4, int64_t(1) << 31, 1, 1}, b) && !mppi_sizes(MppiShape{8, 4, int64_t(1) << 40, 1, 1}, b));
  CHECK(!mppi_sizes(MppiShape{8, 4, 1, int64_t(1) << 62, 1}, b));

  // ---- variant: per block where C >= 64 and E · D · A < 256 · 64
  CHECK(mppi_variant(1, 4096, 8) == kMppiPerBlock && mppi_variant(64, 256, 8) == kMppiPerBlock);
  CHECK(mppi_variant(4096, 4, 8) == kMppiPerThread);
  CHECK(mppi_variant(21, 3, 8) == kMppiPerThread && mppi_variant(1, 300, 8) == kMppiPerBlock);
  CHECK(mppi_variant(1, 63, 8) == kMppiPerThread && mppi_variant(1, 64, 8) == kMppiPerBlock);
  CHECK(mppi_variant(2047, 64, 8) == kMppiPerBlock && mppi_variant(2048, 64, 8) == kMppiPerThread);
  CHECK(mppi_variant(63, 4096, 256) == kMppiPerBlock && mppi_variant(64, 4096, 256) == kMppiPerThread);

  // ---- the row's power of two
  CHECK(mppi_row_pow2(1) == 1 && mppi_row_pow2(2) == 2 && mppi_row_pow2(3) == 4 && mppi_row_pow2(8) == 8);
  CHECK(mppi_row_pow2(12) == 16 && mppi_row_pow2(64) == 64 && mppi_row_pow2(65) == 128 && mppi_row_pow2(256) == 256);
  for (int row = 1; row <= kMppiMaxRow; ++row) {
    const int p = mppi_row_pow2(row);
    CHECK(p >= row && p < 2 * row && (p & (p - 1)) == 0 && kMppiSumThreads % p == 0);
  }

  // ---- grids
  MppiShape s{16, 4096, 1, 8, 1};
  MppiGrids g = mppi_grids(s, mppi_variant(s.E, s.C, s.D * s.A));
  CHECK(g.sample == 4096u * 8 / 256 && g.weights == 1 && g.sum == 16);
  s = MppiShape{16, 4, 4096, 8, 1};
  g = mppi_grids(s, mppi_variant(s.E, s.C, s.D * s.A));
  CHECK(g.sample == 4u * 4096 * 8 / 256 && g.weights == 16 && g.sum == 16u * 4096 * 8 / 256);
  s = MppiShape{7, 5, 21, 3, 4};   // tails: 5 · 21 · 3 = 315 threads a step, 21 envs, 7 · 21 · 12 = 1 764 sums
  g = mppi_grids(s, kMppiPerThread);
  CHECK(g.sample == 2 && g.weights == 1 && g.sum == 7);
  g = mppi_grids(s, kMppiPerBlock);
  CHECK(g.weights == 21 && g.sum == 147);
  s = MppiShape{32, int64_t(1) << 27, 1, 1, 1};   // 2^27 threads a step
  g = mppi_grids(s, kMppiPerBlock);
  CHECK(g.sample == (1u << 19) && g.sum == 32);
  s = MppiShape{8, 1 << 12, 1 << 12, 31, 1};      // the most threads a step: 31 · 2^24 < 2^31
  CHECK(mppi_grids(s, kMppiPerThread).sample == 31u << 16);
  std::printf("mppi_sizes ok\n");
  return 0;
}
