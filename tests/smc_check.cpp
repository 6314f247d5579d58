// Stand-alone host check of csrc/smc_sizes.h (no GPU, no HIP): the byte sizes of a
// particle planner's buffers at two shapes, every refusal bound at its last
// accepted and first refused value, the segment table of a ragged horizon, the
// choice between the two weigh + resample and sum variants and the launch grids.
// Built and run by tests/test_smc_host.py with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "smc_sizes.h"

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  using namespace qs;
  uint64_t b[kSmcBufs];
  // ---- sizes.  n = 64, L = 16 (S = 4), C = 4 096, E = 1, D = 8, A = 1
  CHECK(smc_sizes(SmcShape{64, 16, 4096, 1, 8, 1}, b));
  CHECK(b[kSmcNominal] == 64u * 8 * 4 && b[kSmcCandidates] == 64ull * 4096 * 8 * 4);
  CHECK(b[kSmcBase] == 4096u * 8 && b[kSmcWeights] == 4096u * 8);
  CHECK(b[kSmcParents] == 4u * 4096 * 4 && b[kSmcAncestors] == b[kSmcParents]);
  CHECK(b[kSmcEss] == 4u * 8 && b[kSmcOffset] == 4u * 8 && b[kSmcResampled] == 4u * 4);
  CHECK(b[kSmcBest] == 4 && b[kSmcAction] == 8 * 4 && b[kSmcTick] == 8);
  // n = 40, L = 16 (S = 3, ragged), C = 9, E = 21, D = 3, A = 4
  CHECK(smc_sizes(SmcShape{40, 16, 9, 21, 3, 4}, b));
  CHECK(b[kSmcNominal] == 40u * 21 * 12 * 4 && b[kSmcCandidates] == 40u * 9 * 21 * 12 * 4);
  CHECK(b[kSmcBase] == 189u * 8 && b[kSmcWeights] == 189u * 8 && b[kSmcParents] == 3u * 189 * 4);
  CHECK(b[kSmcAncestors] == 3u * 189 * 4 && b[kSmcEss] == 3u * 21 * 8 && b[kSmcOffset] == 3u * 21 * 8);
  CHECK(b[kSmcResampled] == 3u * 21 * 4 && b[kSmcBest] == 21u * 4 && b[kSmcAction] == 21u * 48 && b[kSmcTick] == 8);

  // ---- the segment table.  n = 40, L = 16: 16, 16, 8
  CHECK(smc_segments(40, 16) == 3);
  CHECK(smc_segment_start(16, 0) == 0 && smc_segment_start(16, 1) == 16 && smc_segment_start(16, 2) == 32);
  CHECK(smc_segment_length(40, 16, 0) == 16 && smc_segment_length(40, 16, 1) == 16 && smc_segment_length(40, 16, 2) == 8);
  CHECK(smc_segments(32, 16) == 2 && smc_segment_length(32, 16, 1) == 16);     // no ragged end
  CHECK(smc_segments(1, 16) == 1 && smc_segment_length(1, 16, 0) == 1);        // n < L
  CHECK(smc_segments(33, 32) == 2 && smc_segment_length(33, 32, 1) == 1);
  CHECK(smc_segments(256, 1) == 256 && smc_segment_length(256, 1, 255) == 1);
  CHECK(!smc_segment_index_ok(40, 16, -1) && smc_segment_index_ok(40, 16, 0) && smc_segment_index_ok(40, 16, 2) &&
        !smc_segment_index_ok(40, 16, 3));

  // ---- refusals, each at its last accepted and first refused value
  // horizon >= 1, at most 256 segments
  CHECK(!smc_sizes(SmcShape{0, 16, 4, 1, 8, 1}, b) && smc_sizes(SmcShape{1, 16, 4, 1, 8, 1}, b));
  CHECK(!smc_sizes(SmcShape{-3, 16, 4, 1, 8, 1}, b));
  CHECK(smc_sizes(SmcShape{256, 1, 4, 1, 8, 1}, b) && !smc_sizes(SmcShape{257, 1, 4, 1, 8, 1}, b));
  CHECK(smc_sizes(SmcShape{256 * 32, 32, 4, 1, 8, 1}, b) && !smc_sizes(SmcShape{256 * 32 + 1, 32, 4, 1, 8, 1}, b));
  CHECK(b[kSmcCandidates] == 8192ull * 4 * 8 * 4 && b[kSmcParents] == 256u * 4 * 4);
  CHECK(smc_sizes(SmcShape{256 * 16 - 15, 16, 4, 1, 8, 1}, b) && !smc_sizes(SmcShape{256 * 16 + 1, 16, 4, 1, 8, 1}, b));
  CHECK(!smc_sizes(SmcShape{std::numeric_limits<int64_t>::max(), 32, 4, 1, 8, 1}, b));
  CHECK(kSmcMaxSegments <= 256);   // the segment has bits 8 .. 15 of the counter word
  // segment 1 .. depth (the handle's depth is at most kMppiMaxSteps = 32)
  CHECK(!smc_sizes(SmcShape{8, 0, 4, 1, 8, 1}, b) && smc_sizes(SmcShape{8, 1, 4, 1, 8, 1}, b));
  CHECK(smc_sizes(SmcShape{64, 32, 4, 1, 8, 1}, b) && !smc_sizes(SmcShape{64, 33, 4, 1, 8, 1}, b));
  CHECK(!smc_segment_ok(0, 32) && smc_segment_ok(1, 32) && smc_segment_ok(32, 32) && !smc_segment_ok(33, 32));
  CHECK(smc_segment_ok(7, 7) && !smc_segment_ok(8, 7) && !smc_segment_ok(1, 0) && !smc_segment_ok(-1, 32));
  // particles 2 .. 4 096
  CHECK(!smc_sizes(SmcShape{8, 8, 1, 1, 8, 1}, b) && smc_sizes(SmcShape{8, 8, 2, 1, 8, 1}, b));
  CHECK(!smc_sizes(SmcShape{8, 8, 0, 1, 8, 1}, b) && !smc_sizes(SmcShape{8, 8, -5, 1, 8, 1}, b));
  CHECK(smc_sizes(SmcShape{8, 8, 4096, 1, 8, 1}, b) && !smc_sizes(SmcShape{8, 8, 4097, 1, 8, 1}, b));
  CHECK(kSmcMaxParticles >= 4096 && kSmcMaxParticles == kSmcBlockThreads * kSmcScanPerThread);
  CHECK(kSmcMaxParticles * 8 + 16 * 12 <= 64 * 1024);   // the weigh workgroup's LDS: cumulative weights and wave partials
  // lo < hi, both finite
  const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
  CHECK(smc_clip_ok(-1.0f, 1.0f) && smc_clip_ok(0.0f, std::nextafter(0.0f, 1.0f)) && !smc_clip_ok(1.0f, 1.0f) &&
        !smc_clip_ok(0.5f, -0.5f));
  CHECK(!smc_clip_ok(-inf, 1.0f) && !smc_clip_ok(0.0f, inf) && !smc_clip_ok(nan, 1.0f) && !smc_clip_ok(0.0f, nan));
  // sigma and done_penalty finite and >= 0
  CHECK(smc_sigma_ok(0.0f) && smc_sigma_ok(3.0f) && !smc_sigma_ok(-std::numeric_limits<float>::denorm_min()) &&
        !smc_sigma_ok(inf) && !smc_sigma_ok(nan) && smc_sigma_ok(std::numeric_limits<float>::max()));
  const double dinf = std::numeric_limits<double>::infinity(), dnan = std::nan("");
  CHECK(smc_penalty_ok(0.0) && smc_penalty_ok(2.5) && !smc_penalty_ok(-std::numeric_limits<double>::denorm_min()) &&
        !smc_penalty_ok(dinf) && !smc_penalty_ok(dnan) && smc_penalty_ok(std::numeric_limits<double>::max()));
  // lambda > 0 and finite
  CHECK(!smc_lambda_ok(0.0) && smc_lambda_ok(std::numeric_limits<double>::denorm_min()) && !smc_lambda_ok(-1.0) &&
        smc_lambda_ok(std::numeric_limits<double>::max()) && !smc_lambda_ok(dinf) && !smc_lambda_ok(dnan));
  // ess_frac in [0, 1]
  CHECK(smc_ess_frac_ok(0.0) && smc_ess_frac_ok(1.0) && smc_ess_frac_ok(0.5) && !smc_ess_frac_ok(std::nextafter(1.0, 2.0)) &&
        !smc_ess_frac_ok(-std::numeric_limits<double>::denorm_min()) && !smc_ess_frac_ok(dnan) && !smc_ess_frac_ok(dinf));
  // envs, drones, components, the row of D · A <= 256
  CHECK(!smc_sizes(SmcShape{8, 8, 4, 0, 8, 1}, b) && !smc_sizes(SmcShape{8, 8, 4, 1, 0, 1}, b));
  CHECK(!smc_sizes(SmcShape{8, 8, 4, 1, 8, 0}, b) && smc_sizes(SmcShape{8, 8, 4, 1, 8, 4}, b) &&
        !smc_sizes(SmcShape{8, 8, 4, 1, 8, 5}, b));
  CHECK(smc_sizes(SmcShape{8, 8, 4, 1, 64, 4}, b) && !smc_sizes(SmcShape{8, 8, 4, 1, 65, 4}, b));
  // the 32-bit offsets of a branch advance: C · E virtual envs, C · E · D virtual agents, a step's actions, ret
  CHECK(!smc_sizes(SmcShape{8, 8, 4096, 1 << 19, 1, 1}, b));                  // C · E = 2^31
  CHECK(smc_sizes(SmcShape{8, 8, 4096, 1 << 15, 1, 1}, b));                   // 2^27 virtual envs, 2^30 B of ret
  CHECK(!smc_sizes(SmcShape{8, 8, 4096, 1 << 16, 1, 1}, b));                  // ret: 2^28 · 8 = 2^31 B
  CHECK(!smc_sizes(SmcShape{8, 8, 4096, 1 << 12, 128, 1}, b));                // C · E · D = 2^31
  CHECK(smc_sizes(SmcShape{8, 8, 4096, 1 << 12, 31, 1}, b));                  // a step: 2^24 · 31 · 4 < 2^31 B
  CHECK(!smc_sizes(SmcShape{8, 8, 4096, 1 << 12, 32, 1}, b));                 // a step: 2^31 B
  CHECK(!smc_sizes(SmcShape{8, 8, 4, int64_t(1) << 31, 1, 1}, b) && !smc_sizes(SmcShape{8, 8, 4, 1, int64_t(1) << 62, 1}, b));
  // the [S][C][E] tables: S · C · E below 2^31
  CHECK(smc_sizes(SmcShape{15, 1, 4096, 1 << 15, 1, 1}, b));                  // 15 · 2^27 < 2^31
  CHECK(b[kSmcParents] == 15ull * (1u << 27) * 4u);
  CHECK(!smc_sizes(SmcShape{16, 1, 4096, 1 << 15, 1, 1}, b));                 // 16 · 2^27 = 2^31

  // ---- variant: mppi_variant's criterion.  The three measured shapes (D = 8, A = 1), then the boundaries
  CHECK(smc_variant(1, 4096, 8) == kSmcPerBlock && smc_variant(64, 256, 8) == kSmcPerBlock);
  CHECK(smc_variant(4096, 4, 8) == kSmcPerThread);
  CHECK(smc_variant(1, 63, 8) == kSmcPerThread && smc_variant(1, 64, 8) == kSmcPerBlock);
  CHECK(smc_variant(2047, 64, 8) == kSmcPerBlock && smc_variant(2048, 64, 8) == kSmcPerThread);
  CHECK(smc_variant(4096, 4096, 8) == kSmcPerThread);
  CHECK(smc_variant(3, 5, 8) == kSmcPerThread && smc_variant(1, 300, 8) == kSmcPerBlock && smc_variant(5, 70, 8) == kSmcPerBlock);
  CHECK(smc_variant(5, 4, 12) == kSmcPerThread && smc_variant(5, 130, 12) == kSmcPerBlock && smc_variant(5, 3, 8) == kSmcPerThread);
  for (int64_t E : {1, 7, 2047, 2048, 100000})
    for (int64_t C : {2, 63, 64, 4096})
      CHECK((smc_variant(E, C, 8) == kSmcPerBlock) == (mppi_variant(E, C, 8) == kMppiPerBlock));

  // ---- grids
  SmcShape s{64, 16, 4096, 1, 8, 1};
  SmcGrids g = smc_grids(s, smc_variant(s.E, s.C, s.D * s.A));
  CHECK(g.begin == 4u * 4096 / 256 && g.sample == 4096u * 8 / 256 && g.weigh == 1 && g.trace == 16 && g.sum == 64);
  s = SmcShape{64, 16, 256, 64, 8, 1};
  g = smc_grids(s, smc_variant(s.E, s.C, s.D * s.A));
  CHECK(g.begin == 4u * 256 * 64 / 256 && g.sample == 256u * 64 * 8 / 256 && g.weigh == 64 && g.trace == 64 && g.sum == 4096);
  s = SmcShape{64, 16, 4, 4096, 8, 1};
  g = smc_grids(s, smc_variant(s.E, s.C, s.D * s.A));
  CHECK(g.begin == 4u * 4 * 4096 / 256 && g.sample == 4u * 4096 * 8 / 256 && g.weigh == 16 && g.trace == 64 &&
        g.sum == 64u * 4096 * 8 / 256);
  s = SmcShape{40, 16, 5, 21, 3, 4};   // tails: 3 · 105 = 315 table entries, 315 threads a step, 21 envs, 40 · 252 elements
  g = smc_grids(s, kSmcPerThread);
  CHECK(g.begin == 2 && g.sample == 2 && g.weigh == 1 && g.trace == 1 && g.sum == 40);
  g = smc_grids(s, kSmcPerBlock);
  CHECK(g.weigh == 21 && g.sum == 840 && g.begin == 2 && g.trace == 1);
  CHECK(smc_grids_fit(s, kSmcPerThread) && smc_grids_fit(s, kSmcPerBlock));
  s = SmcShape{8192, 32, 2, (int64_t(1) << 18) - 1, 1, 1};   // E · n workgroups: below 2^31
  CHECK(smc_grids_fit(s, kSmcPerBlock));
  s.E = int64_t(1) << 18;                                      // 2^13 · 2^18 = 2^31
  CHECK(!smc_grids_fit(s, kSmcPerBlock) && smc_grids_fit(s, kSmcPerThread));
  std::printf("smc_sizes ok\n");
  return 0;
}
