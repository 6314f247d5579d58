// smc_sizes.h — host-side arithmetic of the particle (SMC) planner tick (qs_smc_*;
// plain C++, no HIP).
//
// A planner of horizon n, run in S = ceil(n / L) segments of at most L steps, over
// C particles on a handle with E envs of D drones and A action components owns
// twelve device buffers (and a branch set of C candidates, which sizes itself).
// As for the MPPI and CEM ticks (planner_sizes.h, whose per-step bounds it shares)
// the plain arithmetic lives here: the bytes of every buffer and whether the shape
// and the spec's numbers can be planned, the segment table, which of the two
// weigh + resample and sum variants runs, and the grids of the launches.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "planner_sizes.h"

namespace qs {

constexpr int kSmcTag = 5;                // Philox domain tag of the particles' noise (3: MPPI, 4: CEM)
constexpr int kSmcOffsetTag = 6;          // ... and of the resampling offset u, one draw per (tick, env, segment)
constexpr int kSmcThreads = kPlannerThreads;             // begin, sample, trace and the per-thread variants
constexpr int kSmcBlockThreads = kPlannerBlockThreads;   // the per-workgroup weigh + resample and sum
constexpr int kSmcMaxSegments = 256;      // S at most: the counter word gives the segment bits 8 .. 15
constexpr int kSmcScanPerThread = 4;      // particles a thread of the per-workgroup scan holds at most
// C at most: the per-workgroup variant keeps an env's cumulative weights in LDS,
// one double a particle (32 KB), kSmcScanPerThread of them to a thread.
constexpr int kSmcMaxParticles = kSmcBlockThreads * kSmcScanPerThread;   // 4 096

// The planner's buffers, in qs_smc_bufs' order.
enum { kSmcNominal = 0, kSmcCandidates, kSmcBase, kSmcWeights, kSmcParents, kSmcAncestors, kSmcEss, kSmcOffset,
       kSmcResampled, kSmcBest, kSmcAction, kSmcTick, kSmcBufs };

struct SmcShape {
  int64_t n, L, C, E, D, A;
};

// Segments of a horizon: S = ceil(n / L); segment s starts at step s · L and holds
// L steps, the last one what is left (1 .. L).
inline int64_t smc_segments(int64_t n, int64_t L) { return (n + L - 1) / L; }
inline int64_t smc_segment_start(int64_t L, int64_t s) { return s * L; }
inline int64_t smc_segment_length(int64_t n, int64_t L, int64_t s) {
  const int64_t left = n - s * L;
  return left < L ? left : L;
}

// Bytes of every buffer; false where the shape cannot be planned: n < 1, L
// outside 1 .. kMppiMaxSteps (the caller holds it to the handle's own depth),
// more than kSmcMaxSegments segments, C outside 2 .. kSmcMaxParticles, whatever
// mppi_sizes refuses for one segment of (L, C, E, D, A) (the row width and the
// 32-bit offsets of a branch advance), or a [S][C][E] table of 2^31 entries or more.
inline bool smc_sizes(const SmcShape& s, uint64_t b[kSmcBufs]) {
  if (s.n < 1 || s.L < 1 || s.L > kMppiMaxSteps) return false;
  if (s.n > (int64_t)kSmcMaxSegments * s.L) return false;       // (before the division: n is any int64)
  const uint64_t S = (uint64_t)smc_segments(s.n, s.L);          // 1 .. 256
  if (s.C < 2 || s.C > kSmcMaxParticles) return false;
  uint64_t m[kMppiBufs];
  if (!mppi_sizes(MppiShape{s.L, s.C, s.E, s.D, s.A}, m)) return false;
  const uint64_t V = (uint64_t)s.C * (uint64_t)s.E;             // < 2^31 (mppi_sizes)
  if (S * V >= (uint64_t(1) << 31)) return false;
  const uint64_t col = m[kMppiAction];                          // E · D · A · 4 bytes
  b[kSmcNominal] = (uint64_t)s.n * col;                         // n <= 8 192, col < 2^31
  b[kSmcCandidates] = (uint64_t)s.n * (m[kMppiCandidates] / (uint64_t)s.L);
  b[kSmcBase] = V * 8u;
  b[kSmcWeights] = V * 8u;
  b[kSmcParents] = S * V * 4u;
  b[kSmcAncestors] = S * V * 4u;
  b[kSmcEss] = S * (uint64_t)s.E * 8u;
  b[kSmcOffset] = S * (uint64_t)s.E * 8u;
  b[kSmcResampled] = S * (uint64_t)s.E * 4u;
  b[kSmcBest] = (uint64_t)s.E * 4u;
  b[kSmcAction] = col;
  b[kSmcTick] = 8u;
  return true;
}

// The spec's numbers, each with the bound it is refused at.
inline bool smc_lambda_ok(double lambda) { return lambda > 0.0 && std::isfinite(lambda); }
inline bool smc_penalty_ok(double p) { return p >= 0.0 && std::isfinite(p); }
inline bool smc_sigma_ok(float s) { return s >= 0.0f && std::isfinite(s); }
inline bool smc_clip_ok(float lo, float hi) { return lo < hi && std::isfinite(lo) && std::isfinite(hi); }
inline bool smc_ess_frac_ok(double f) { return f >= 0.0 && f <= 1.0; }   // (false for a NaN)
inline bool smc_segment_ok(int64_t L, int64_t depth) { return L >= 1 && L <= depth; }
inline bool smc_segment_index_ok(int64_t n, int64_t L, int64_t s) { return s >= 0 && s < smc_segments(n, L); }

// Which weigh + resample and which sum runs: mppi_variant's criterion.
//  kSmcPerThread: one thread per env loops over the particles (weights, then a
//    merge walk of the C positions along the running cumulative weight); the sum
//    by one thread per (step, env, drone, component) looping over c.
//  kSmcPerBlock: a workgroup per env (at most kSmcScanPerThread particles a
//    thread, a block scan of the weights into LDS and a binary search per
//    position); the sum by a workgroup per (env, step).
enum SmcVariant { kSmcPerThread = 0, kSmcPerBlock = 1 };
inline SmcVariant smc_variant(int64_t E, int64_t C, int64_t row) {
  return mppi_variant(E, C, row) == kMppiPerBlock ? kSmcPerBlock : kSmcPerThread;
}

// Grids (workgroups) of the launches.  begin, sample, weigh and trace stay below
// 2^31 by smc_sizes (S · C · E < 2^31, C · E · D < 2^31); the sum's grid grows with
// n <= 8 192 and has a check of its own, smc_grids_fit.  Every factor is bounded
// by smc_sizes, so the 64-bit products cannot overflow.
struct SmcGrids {
  uint32_t begin;     // kSmcThreads threads, one per (s, c, e) of parents
  uint32_t sample;    // x of a (sample, segment length) grid, kSmcThreads threads each: one per (c, e, d) of a step
  uint32_t weigh;     // per thread: kSmcThreads threads, one per env; per block: kSmcBlockThreads, one workgroup per env
  uint32_t trace;     // kSmcThreads threads, one per (c, e)
  uint32_t sum;       // per thread: kSmcThreads threads, one per (j, e, d, a); per block: kSmcBlockThreads, one per (e, j)
};
inline SmcGrids smc_grids(const SmcShape& s, SmcVariant v) {
  SmcGrids g;
  const uint64_t S = (uint64_t)smc_segments(s.n, s.L);
  g.begin = mppi_div_up(S * (uint64_t)s.C * (uint64_t)s.E, kSmcThreads);
  g.sample = mppi_div_up((uint64_t)s.C * s.E * s.D, kSmcThreads);
  g.trace = mppi_div_up((uint64_t)s.C * s.E, kSmcThreads);
  if (v == kSmcPerBlock) {
    g.weigh = (uint32_t)s.E;
    g.sum = (uint32_t)((uint64_t)s.E * (uint64_t)s.n);
  } else {
    g.weigh = mppi_div_up((uint64_t)s.E, kSmcThreads);
    g.sum = mppi_div_up((uint64_t)s.n * s.E * s.D * s.A, kSmcThreads);
  }
  return g;
}
// Whether the sum's grid fits: E · n workgroups (per block) or n · E · D · A /
// kSmcThreads (per thread) below 2^31.
inline bool smc_grids_fit(const SmcShape& s, SmcVariant v) {
  const uint64_t lim = uint64_t(1) << 31;
  if (v == kSmcPerBlock) return (uint64_t)s.E * (uint64_t)s.n < lim;
  return ((uint64_t)s.n * s.E * s.D * s.A + kSmcThreads - 1) / kSmcThreads < lim;
}

}  // namespace qs
