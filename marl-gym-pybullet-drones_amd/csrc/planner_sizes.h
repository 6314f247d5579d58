// planner_sizes.h — host-side arithmetic of the MPPI planner tick (qs_mppi_*; plain
// C++, no HIP).
//
// A planner of horizon n over C candidates on a handle with E envs of D drones
// and A action components owns eight device buffers.  Three decisions are plain
// arithmetic and live here: how many bytes each buffer takes and whether the
// shape is one qs_score (and the sample kernel's Philox counter) can take, which
// of the two reduction variants the update runs, and the grids of the launches.
// A planner in per-drone mode (qs_pd_mppi_create) has the same buffers with a drone
// axis on weights and best, plus ret_agent: mppi_pd_shape and mppi_pd_sizes below.
#pragma once

#include <cstddef>
#include <cstdint>

namespace qs {

constexpr int kMppiMaxSteps = 32;          // = kScoreMaxSteps (step_score.h): the counter word holds c · 32 + j
constexpr int kMppiTag = 3;                // Philox domain tag of the planner's noise (1: actions, 2: reset tries)
constexpr int kPlannerThreads = 256;       // workgroup of the sample kernel and of both planners' per-thread variants
constexpr int kPlannerBlockThreads = 1024; // workgroup of both planners' per-workgroup variants (16 waves)
constexpr int kMppiThreads = kPlannerThreads;
constexpr int kMppiSumThreads = kPlannerBlockThreads;   // the per-workgroup weights and weighted sum
constexpr int kMppiMaxRow = 256;           // D · A at most (D <= 64, A <= 4)
constexpr int64_t kMppiMaxCandidates = int64_t(1) << 27;   // c · 32 + j stays inside one 32-bit counter word

// The planner's buffers, in qs_mppi_bufs' order.
enum { kMppiNominal = 0, kMppiCandidates, kMppiRet, kMppiFirstDone, kMppiWeights, kMppiBest, kMppiAction, kMppiTick,
       kMppiBufs };

struct MppiShape {
  int64_t n, C, E, D, A;
};

// Bytes of every buffer; false where the shape cannot be planned: a horizon
// outside 1 .. kMppiMaxSteps, fewer than two candidates or more than the counter
// word holds, a row wider than kMppiMaxRow, or sizes beyond the 32-bit offsets
// qs_score refuses (C · E · D virtual agents below 2^31, a step's candidate
// actions and ret / first_done below 2^31 bytes).  The whole candidates buffer
// may pass 2^31 bytes (n steps of up to 2^31 each): the kernels index it in 64 bits.
inline bool mppi_sizes(const MppiShape& s, uint64_t b[kMppiBufs]) {
  if (s.n < 1 || s.n > kMppiMaxSteps || s.C < 2 || s.C > kMppiMaxCandidates) return false;
  if (s.E < 1 || s.D < 1 || s.A < 1 || s.A > 4) return false;
  const uint64_t lim = uint64_t(1) << 31;
  if ((uint64_t)s.E >= lim || (uint64_t)s.D >= lim) return false;
  const uint64_t row = (uint64_t)s.D * (uint64_t)s.A;           // D < 2^31, A <= 4
  if (row > (uint64_t)kMppiMaxRow) return false;
  const uint64_t V = (uint64_t)s.C * (uint64_t)s.E;             // C <= 2^27, E < 2^31
  if (V >= lim) return false;
  if (V * (uint64_t)s.D >= lim) return false;                   // V < 2^31, D <= 256
  const uint64_t step = V * row * 4u;                           // V < 2^31, row <= 256
  if (step >= lim || V * 8u >= lim) return false;
  const uint64_t nom = (uint64_t)s.n * (uint64_t)s.E * row * 4u;   // <= step · 32 / C
  b[kMppiNominal] = nom;
  b[kMppiCandidates] = (uint64_t)s.n * step;
  b[kMppiRet] = V * 8u;
  b[kMppiFirstDone] = V * 4u;
  b[kMppiWeights] = V * 8u;
  b[kMppiBest] = (uint64_t)s.E * 4u;
  b[kMppiAction] = (uint64_t)s.E * row * 4u;
  b[kMppiTick] = 8u;
  return true;
}

// Per-drone mode (qs_pd_mppi_create): the update treats agent (e, d) as env-level
// planning treats env e, so it runs over E · D "envs" with rows of A components
// and the same memory.  The shape the variant and the update's grids are taken from:
inline MppiShape mppi_pd_shape(const MppiShape& s) { return MppiShape{s.n, s.C, s.E * s.D, 1, s.A}; }
// Bytes of every buffer in per-drone mode and of the planner's ret_agent
// ([C][E][D] doubles): weights grow to [C][E][D], best to [E][D], the rest is
// mppi_sizes'.  false where mppi_sizes refuses the shape, where ret_agent would
// pass the 32-bit offsets of qs_score_agents (C · E · D · 8 bytes below 2^31), or
// where the update's workgroup-per-(agent, step) grid would pass 2^31.  Every
// product is formed in 64 bits from factors mppi_sizes has bounded.
inline bool mppi_pd_sizes(const MppiShape& s, uint64_t b[kMppiBufs], uint64_t* ret_agent) {
  if (!mppi_sizes(s, b)) return false;                          // C · E · D < 2^31, n <= 32
  const uint64_t lim = uint64_t(1) << 31;
  const uint64_t agents = (uint64_t)s.E * (uint64_t)s.D;        // < 2^31 (C >= 2)
  const uint64_t N = (uint64_t)s.C * agents;                    // < 2^31
  if (N * 8u >= lim) return false;
  if ((uint64_t)s.n * agents >= lim) return false;              // n <= 32
  b[kMppiWeights] = N * 8u;
  b[kMppiBest] = agents * 4u;
  *ret_agent = N * 8u;
  return true;
}

// Which reduction the update runs.
//  kMppiPerThread: weights by one thread per env looping over c, the weighted
//    sum by one thread per (step, env, drone, component) looping over c; reads
//    are coalesced across the envs.  Right for many envs and few candidates.
//  kMppiPerBlock: weights by a workgroup per env, the weighted sum by a
//    workgroup per (env, step), both striding over c and finishing with an
//    in-wave tree and an LDS tree.  Right where a step of all envs would not
//    give every compute unit a wave of per-thread work (E · D · A below 256 CUs ·
//    64 lanes) and a workgroup's wave still finds a candidate per lane (C >= 64).
enum MppiVariant { kMppiPerThread = 0, kMppiPerBlock = 1 };
constexpr int64_t kMppiBlockMinC = 64;
constexpr int64_t kMppiBlockMaxRowsElems = 256 * 64;
inline MppiVariant mppi_variant(int64_t E, int64_t C, int64_t row) {
  return (C >= kMppiBlockMinC && E * row < kMppiBlockMaxRowsElems) ? kMppiPerBlock : kMppiPerThread;
}

// Smallest power of two >= row (row in 1 .. kMppiMaxRow): the per-workgroup sum
// lays a candidate's row out over that many lanes, so lanes of one component sit
// a power of two apart and the in-wave tree is plain xor steps.
inline int mppi_row_pow2(int64_t row) {
  int p = 1;
  while (p < row) p <<= 1;
  return p;
}

inline uint32_t mppi_div_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// Grids (workgroups) of the launches.  All stay below 2^31: C · E · D < 2^31.
struct MppiGrids {
  uint32_t sample;    // x of a (sample, n) grid, kMppiThreads threads each: one thread per (c, e, d) of a step, so
                      // that the kernel's index arithmetic stays in 32 bits
  uint32_t weights;   // per thread: kMppiThreads threads, one per env; per block: kMppiSumThreads, one workgroup per env
  uint32_t sum;       // per thread: kMppiThreads threads, one per (j, e, d, a); per block: kMppiSumThreads, one workgroup per (e, j)
};
inline MppiGrids mppi_grids(const MppiShape& s, MppiVariant v) {
  MppiGrids g;
  g.sample = mppi_div_up((uint64_t)s.C * s.E * s.D, kMppiThreads);
  if (v == kMppiPerBlock) {
    g.weights = (uint32_t)s.E;
    g.sum = (uint32_t)(s.E * s.n);
  } else {
    g.weights = mppi_div_up((uint64_t)s.E, kMppiThreads);
    g.sum = mppi_div_up((uint64_t)s.n * s.E * s.D * s.A, kMppiThreads);
  }
  return g;
}

}  // namespace qs
