// Stand-alone host check of csrc/sampling_sizes.h (no GPU, no HIP): every refusal of
// a sampling spec at its boundary values, the noise scale, the byte size of `kept`
// with its 32-bit-offset bound at the last accepted and first refused value, and
// the grids of the launches the spec changes at the three reference shapes and at a
// 105-thread shape.  Built and run by tests/test_sampling_host.py with
// -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "sampling_sizes.h"
#include "cem_sizes.h"
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
  CHECK(kSamplingThreads == kPlannerThreads && kSamplingMaxAct == 4);

  // ---- rho.  [0, 1): -0.0 is 0; 1, anything above, anything below 0, NaN and the infinities are out
  const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
  const float under1 = std::nextafterf(1.0f, 0.0f), below0 = -std::numeric_limits<float>::denorm_min();
  for (float r : {0.0f, -0.0f, std::numeric_limits<float>::denorm_min(), 0.5f, 0.9f, 0.99f, under1}) CHECK(sampling_rho_ok(r));
  for (float r : {1.0f, std::nextafterf(1.0f, 2.0f), 2.0f, below0, -0.5f, -1.0f, inf, -inf, nan, -nan}) CHECK(!sampling_rho_ok(r));
  // the scale: formed in double, rounded once
  CHECK(sampling_scale(0.0f) == 1.0f && sampling_scale(-0.0f) == 1.0f);
  CHECK(sampling_scale(0.5f) == (float)std::sqrt(0.75));
  CHECK(sampling_scale(0.9f) == (float)std::sqrt(1.0 - (double)0.9f * (double)0.9f));
  CHECK(sampling_scale(under1) > 0.0f && sampling_scale(under1) < 1e-3f);
  for (float r : {0.1f, 0.5f, 0.9f, 0.99f, under1}) {   // unit variance: rho^2 + s^2 = 1 to float rounding
    const double s = sampling_scale(r);
    CHECK(std::fabs((double)r * r + s * s - 1.0) < 2e-7);
  }

  // ---- refusals, in the order of the checks.  CEM: n = 16, C = 9, K = 4, no prior, E = 5, D = 8, A = 1
  const SamplingShape cem{kSamplingCem, 16, 9, 4, 0, 5, 8, 1};
  const SamplingShape mppi{kSamplingMppi, 16, 9, 0, 0, 5, 8, 1};
  const SamplingShape smc{kSamplingSmc, 40, 9, 0, 0, 5, 8, 1};
  const SamplingSpecShape zero{{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0};
  for (const SamplingShape& s : {cem, mppi, smc}) CHECK(sampling_refusal(zero, s) == kSamplingOk);
  SamplingSpecShape v = zero;
  for (const SamplingShape& s : {cem, mppi, smc}) {
    for (float r : {under1, -0.0f, 0.9f}) { v = zero; v.rho[0] = r; CHECK(sampling_refusal(v, s) == kSamplingOk); }
    for (float r : {1.0f, nan, inf, below0, -1.0f}) { v = zero; v.rho[0] = r; CHECK(sampling_refusal(v, s) == kSamplingRho); }
    // components from A on are not read
    for (float r : {1.0f, nan, -1.0f}) { v = zero; v.rho[1] = r; v.rho[3] = r; CHECK(sampling_refusal(v, s) == kSamplingOk); }
  }
  const SamplingShape cem4{kSamplingCem, 16, 9, 4, 0, 7, 3, 4};
  for (int a = 0; a < 4; ++a) {
    v = zero; v.rho[a] = 1.0f; CHECK(sampling_refusal(v, cem4) == kSamplingRho);
    v = zero; v.rho[a] = nan; CHECK(sampling_refusal(v, cem4) == kSamplingRho);
    v = zero; v.rho[a] = under1; CHECK(sampling_refusal(v, cem4) == kSamplingOk);
  }
  v = zero; v.rho[0] = 1.0f; v.reserved = 1; v.keep = -1; CHECK(sampling_refusal(v, cem) == kSamplingRho);   // the order
  for (int64_t r : {int64_t(1), int64_t(-1), int64_t(1) << 31}) { v = zero; v.reserved = r; CHECK(sampling_refusal(v, cem) == kSamplingReserved); }
  v = zero; v.reserved = 1; v.keep = -1; CHECK(sampling_refusal(v, cem) == kSamplingReserved);
  for (const SamplingShape& s : {cem, mppi, smc}) { v = zero; v.keep = -1; CHECK(sampling_refusal(v, s) == kSamplingKeepNeg); }
  for (const SamplingShape& s : {mppi, smc}) {
    for (int64_t k : {int64_t(1), int64_t(2), int64_t(1) << 40}) { v = zero; v.keep = k; CHECK(sampling_refusal(v, s) == kSamplingKeepKind); }
  }
  // keep == elites and keep == elites + 1
  v = zero; v.keep = 4; CHECK(sampling_refusal(v, cem) == kSamplingOk);
  v = zero; v.keep = 5; CHECK(sampling_refusal(v, cem) == kSamplingKeepElites);
  v = zero; v.keep = 1; CHECK(sampling_refusal(v, SamplingShape{kSamplingCem, 16, 9, 1, 0, 5, 8, 1}) == kSamplingOk);
  v = zero; v.keep = 2; CHECK(sampling_refusal(v, SamplingShape{kSamplingCem, 16, 9, 1, 0, 5, 8, 1}) == kSamplingKeepElites);
  // 1 + keep + count == C and == C + 1
  v = zero; v.keep = 2;
  CHECK(sampling_refusal(v, SamplingShape{kSamplingCem, 16, 9, 4, 6, 5, 8, 1}) == kSamplingOk);       // 1 + 2 + 6 = 9
  CHECK(sampling_refusal(v, SamplingShape{kSamplingCem, 16, 9, 4, 7, 5, 8, 1}) == kSamplingSlots);    // 1 + 2 + 7 = 10
  v.keep = 4;
  CHECK(sampling_refusal(v, SamplingShape{kSamplingCem, 16, 9, 4, 4, 5, 8, 1}) == kSamplingOk);
  CHECK(sampling_refusal(v, SamplingShape{kSamplingCem, 16, 9, 4, 5, 5, 8, 1}) == kSamplingSlots);
  // elites = C: without a prior keep may reach C - 1, not C
  v = zero; v.keep = 8; CHECK(sampling_refusal(v, SamplingShape{kSamplingCem, 16, 9, 9, 0, 5, 8, 1}) == kSamplingOk);
  v = zero; v.keep = 9; CHECK(sampling_refusal(v, SamplingShape{kSamplingCem, 16, 9, 9, 0, 5, 8, 1}) == kSamplingSlots);
  CHECK(sampling_slots_ok(9, 2, 6) && !sampling_slots_ok(9, 2, 7) && sampling_slots_ok(9, 0, 8) && !sampling_slots_ok(9, 0, 9));
  CHECK(sampling_slots_ok(2, 0, 1) && sampling_slots_ok(2, 1, 0) && !sampling_slots_ok(2, 1, 1) && !sampling_slots_ok(0, 0, 0));
  CHECK(!sampling_slots_ok(9, -1, 0) && !sampling_slots_ok(9, 0, -1));
  const int64_t big = std::numeric_limits<int64_t>::max();
  CHECK(!sampling_slots_ok(big, big, big) && sampling_slots_ok(big, big - 1, 0) && !sampling_slots_ok(big, big, 0));

  // ---- kept.  [n][keep][E][D][A] f32; a step of it below 2^31 bytes
  uint64_t b = 0;
  CHECK(sampling_kept_bytes(16, 2, 5, 8, 1, &b) && b == 16ull * 2 * 5 * 8 * 4);
  CHECK(sampling_kept_bytes(7, 3, 7, 3, 4, &b) && b == 7ull * 3 * 7 * 3 * 4 * 4);
  CHECK(sampling_kept_bytes(16, 0, 5, 8, 1, &b) && b == 0);
  CHECK(!sampling_kept_bytes(0, 2, 5, 8, 1, &b) && sampling_kept_bytes(1, 2, 5, 8, 1, &b));
  CHECK(sampling_kept_bytes(32, 2, 5, 8, 1, &b) && !sampling_kept_bytes(33, 2, 5, 8, 1, &b));
  CHECK(!sampling_kept_bytes(16, -1, 5, 8, 1, &b) && !sampling_kept_bytes(16, 2, 0, 8, 1, &b));
  CHECK(!sampling_kept_bytes(16, 2, 5, 0, 1, &b) && !sampling_kept_bytes(16, 2, 5, 8, 0, &b));
  CHECK(sampling_kept_bytes(16, 2, 5, 8, 4, &b) && !sampling_kept_bytes(16, 2, 5, 8, 5, &b));
  CHECK(sampling_kept_bytes(16, 2, 5, 64, 4, &b) && !sampling_kept_bytes(16, 2, 5, 65, 4, &b));   // D · A <= 256
  // D = 8, A = 1: keep · E · 32 bytes below 2^31, keep · E up to 2^26 - 1
  CHECK(sampling_kept_bytes(32, 1024, 65535, 8, 1, &b) && b == 32ull * 1024 * 65535 * 32);
  CHECK(sampling_kept_bytes(32, 1, (1 << 26) - 1, 8, 1, &b) && b == 32ull * ((1ull << 26) - 1) * 32);
  CHECK(!sampling_kept_bytes(32, 1, 1 << 26, 8, 1, &b) && !sampling_kept_bytes(32, 1024, 65536, 8, 1, &b));
  // factors that would wrap a 64-bit product
  CHECK(!sampling_kept_bytes(16, int64_t(1) << 40, int64_t(1) << 40, 8, 1, &b));
  CHECK(!sampling_kept_bytes(16, 2, 5, int64_t(1) << 62, 4, &b));
  // ... as a refusal: the last check, and only with keep > 0
  v = zero; v.keep = 1024;
  CHECK(sampling_refusal(v, SamplingShape{kSamplingCem, 32, 2048, 1024, 0, 65535, 8, 1}) == kSamplingOk);
  CHECK(sampling_refusal(v, SamplingShape{kSamplingCem, 32, 2048, 1024, 0, 65536, 8, 1}) == kSamplingOffsets);
  v = zero; v.rho[0] = 0.9f;
  CHECK(sampling_refusal(v, SamplingShape{kSamplingCem, 32, 2048, 1024, 0, 65536, 8, 1}) == kSamplingOk);
  CHECK(sampling_refusal(v, smc) == kSamplingOk);   // a particle planner's horizon is not held to 32 steps

  // ---- which sample kernel runs
  const float r0[4] = {0.0f, -0.0f, 0.0f, 0.0f}, r1[4] = {0.0f, 0.0f, 0.0f, 0.5f}, r2[4] = {0.9f, 0.0f, 0.0f, 0.0f};
  CHECK(!sampling_correlated(r0, 4) && sampling_correlated(r1, 4) && !sampling_correlated(r1, 3) && sampling_correlated(r2, 1));

  // ---- grids at the three reference shapes (D = 8, A = 1, n = 16) and at 105 threads (E = 7, D = 3, C = 5, A = 4)
  struct Ref { int64_t E, C, K; uint32_t sample; };
  for (const Ref& r : {Ref{1, 4096, 64, 128}, Ref{64, 256, 32, 512}, Ref{4096, 4, 2, 512}}) {
    const CemShape cs{16, r.C, r.K, 3, r.E, 8, 1};
    const uint32_t g = sampling_sample_grid(r.C, r.E, 8);
    CHECK(g == r.sample);
    // x of the (sample, n) grid the serial launch replaces, whoever the planner is
    CHECK(g == cem_grids(cs, cem_variant(r.E, r.C, 8)).sample);
    CHECK(g == mppi_grids(MppiShape{16, r.C, r.E, 8, 1}, mppi_variant(r.E, r.C, 8)).sample);
    CHECK((uint64_t)g * kSamplingThreads >= (uint64_t)r.C * r.E * 8 && (uint64_t)(g - 1) * kSamplingThreads < (uint64_t)r.C * r.E * 8);
    const int64_t keep = r.K / 2;
    const uint32_t k = sampling_finish_grid(keep, r.E, 8, 1);   // the mean's columns, then kept's
    CHECK((uint64_t)k * kSamplingThreads >= (uint64_t)(keep + 1) * r.E * 8 && (uint64_t)(k - 1) * kSamplingThreads < (uint64_t)(keep + 1) * r.E * 8);
    CHECK(k >= cem_grids(cs, cem_variant(r.E, r.C, 8)).finish && sampling_finish_grid(0, r.E, 8, 1) == cem_grids(cs, cem_variant(r.E, r.C, 8)).finish);
    v = zero; v.rho[0] = 0.9f; v.keep = keep;
    CHECK(sampling_refusal(v, SamplingShape{kSamplingCem, 16, r.C, r.K, 0, r.E, 8, 1}) == kSamplingOk);
  }
  CHECK(sampling_finish_grid(32, 1, 8, 1) == 2 && sampling_finish_grid(16, 64, 8, 1) == 34 && sampling_finish_grid(1, 4096, 8, 1) == 256);
  CHECK(sampling_sample_grid(5, 7, 3) == 1 && sampling_finish_grid(2, 7, 3, 4) == 1);        // 105 threads; 84 + 168 columns
  CHECK(sampling_sample_grid(9, 5, 8) == 2 && sampling_finish_grid(2, 5, 8, 1) == 1);        // 360 threads: a partial second workgroup
  CHECK(sampling_sample_grid(1, 1, 1) == 1 && sampling_sample_grid(256, 1, 1) == 1 && sampling_sample_grid(257, 1, 1) == 2);
  CHECK(sampling_finish_grid(3, 8, 8, 1) == 1 && sampling_finish_grid(4, 8, 8, 1) == 2 && sampling_finish_grid(0, 1, 1, 1) == 1);
  CHECK(sampling_sample_grid(9, 5, 8) == smc_grids(SmcShape{40, 16, 9, 5, 8, 1}, smc_variant(5, 9, 8)).sample);
  std::printf("sampling_sizes ok\n");
  return 0;
}
