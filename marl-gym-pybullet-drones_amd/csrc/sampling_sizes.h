// sampling_sizes.h — host-side arithmetic of the sampling spec (qs_sampling_mppi_set /
// qs_sampling_cem_set / qs_sampling_smc_set; plain C++, no HIP).
//
// A sampling spec gives the planners' shared sample stage an AR(1) coefficient per
// action component and, for the CEM tick, `keep` elites carried from one refit to the
// next sample.  What is plain arithmetic lives here: which specs are refused, the
// noise scale s = sqrt(1 - rho^2), the bytes of the `kept` buffer with its 32-bit-offset
// bound, and the grids of the two launches the spec changes: the serial-in-j sample
// kernel, and the CEM finish launch, which with an elite memory also shifts `kept`
// (the refit and sample kernels take the elite memory in their own grids).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "planner_sizes.h"

namespace qs {

constexpr int kSamplingThreads = kPlannerThreads;   // workgroup of every launch below
constexpr int kSamplingMaxAct = 4;                   // A at most: the four normals of one Philox draw

// Which planner a spec is attached to: only the CEM tick has elites to keep.
enum SamplingKind { kSamplingMppi = 0, kSamplingCem, kSamplingSmc };

// Why a sampling spec is refused (0: it is not).  The order is the order of the checks.
enum SamplingRefusal {
  kSamplingOk = 0,
  kSamplingRho,        // rho[a] outside [0, 1) or not finite, for some a < A
  kSamplingReserved,   // reserved != 0
  kSamplingKeepNeg,    // keep < 0
  kSamplingKeepKind,   // keep != 0 on an MPPI or particle planner
  kSamplingKeepElites, // keep > elites
  kSamplingSlots,      // 1 + keep + prior count > candidates: the mean, the kept and the prior slots would overlap
  kSamplingOffsets,    // a step of `kept` (keep · E · D · A · 4 bytes) at or past 2^31
};

struct SamplingSpecShape {
  float rho[kSamplingMaxAct];
  int64_t keep, reserved;
};

// The planner a spec is held against: n steps, C candidates, K elites (CEM; 0
// otherwise), `prior` candidates of an attached policy prior (0: none), E envs of D
// drones and A action components.
struct SamplingShape {
  SamplingKind kind;
  int64_t n, C, K, prior, E, D, A;
};

// rho in [0, 1): -0.0 is 0, a NaN fails both comparisons.
inline bool sampling_rho_ok(float rho) { return rho >= 0.0f && rho < 1.0f; }

// s = (float)sqrt(1 - (double)rho^2): what the fresh normal is scaled by, so that the
// recurrence keeps unit variance.
inline float sampling_scale(float rho) { return (float)std::sqrt(1.0 - (double)rho * (double)rho); }

// Slot 0 is the mean, slots 1 .. keep the elite memory, the last `prior` slots the
// policy prior's: they fit side by side in C candidates.
inline bool sampling_slots_ok(int64_t C, int64_t keep, int64_t prior) {
  if (keep < 0 || prior < 0 || C < 1) return false;
  return prior <= C - 1 && keep <= C - 1 - prior;   // (no sum that could wrap)
}

// Bytes of kept [n][keep][E][D][A] f32 (0 with keep = 0).  false where the shape is
// outside what the launches index: n outside 1 .. kMppiMaxSteps, an empty or negative
// axis, A above kSamplingMaxAct, D · A above kMppiMaxRow, or one step of kept rows at
// or past 2^31 bytes.  Every product is formed in 64 bits from factors bounded first.
inline bool sampling_kept_bytes(int64_t n, int64_t keep, int64_t E, int64_t D, int64_t A, uint64_t* bytes) {
  const uint64_t lim = uint64_t(1) << 31;
  if (n < 1 || n > kMppiMaxSteps || keep < 0 || E < 1 || D < 1 || A < 1 || A > kSamplingMaxAct) return false;
  if ((uint64_t)keep >= lim || (uint64_t)E >= lim || (uint64_t)D >= lim) return false;
  const uint64_t row = (uint64_t)D * (uint64_t)A;             // D < 2^31, A <= 4
  if (row > (uint64_t)kMppiMaxRow) return false;
  const uint64_t V = (uint64_t)keep * (uint64_t)E;            // < 2^62
  if (V >= lim) return false;
  const uint64_t step = V * row * 4u;                         // V < 2^31, row <= 256
  if (step >= lim) return false;
  *bytes = (uint64_t)n * step;                                // n <= 32
  return true;
}

// The checks of a sampling spec against the planner it is attached to, in the order
// of SamplingRefusal.
inline SamplingRefusal sampling_refusal(const SamplingSpecShape& v, const SamplingShape& s) {
  for (int a = 0; a < kSamplingMaxAct && a < s.A; ++a)
    if (!sampling_rho_ok(v.rho[a])) return kSamplingRho;
  if (v.reserved != 0) return kSamplingReserved;
  if (v.keep < 0) return kSamplingKeepNeg;
  if (v.keep != 0 && s.kind != kSamplingCem) return kSamplingKeepKind;
  if (v.keep > s.K) return kSamplingKeepElites;
  if (!sampling_slots_ok(s.C, v.keep, s.prior)) return kSamplingSlots;
  uint64_t bytes;
  if (v.keep != 0 && !sampling_kept_bytes(s.n, v.keep, s.E, s.D, s.A, &bytes)) return kSamplingOffsets;
  return kSamplingOk;
}

// Whether the serial-in-j sample kernel replaces the (sample, n) launch: some
// component among the first A has a non-zero rho.
inline bool sampling_correlated(const float rho[kSamplingMaxAct], int64_t A) {
  for (int a = 0; a < kSamplingMaxAct && a < A; ++a)
    if (rho[a] != 0.0f) return true;
  return false;
}

// Grid of the serial-in-j sample kernel, kSamplingThreads threads a workgroup: one
// thread per (c, e, d), which walks the steps.  It is x of the (sample, n) grid it
// replaces (MppiGrids / CemGrids / SmcGrids .sample).
inline uint32_t sampling_sample_grid(int64_t C, int64_t E, int64_t D) {
  return mppi_div_up((uint64_t)C * (uint64_t)E * (uint64_t)D, kSamplingThreads);
}

// Grid of the CEM finish launch with an elite memory, kSamplingThreads threads a
// workgroup: one thread per (e, d, a) column of the mean and, after those, one per
// (r, e, d, a) column of kept; each walks the steps upward.  (1 + keep) · E · D · A
// stays below 2^31: keep < C, and a step of candidates is below 2^31 bytes.
inline uint32_t sampling_finish_grid(int64_t keep, int64_t E, int64_t D, int64_t A) {
  return mppi_div_up(((uint64_t)keep + 1u) * (uint64_t)E * (uint64_t)D * (uint64_t)A, kSamplingThreads);
}

}  // namespace qs
