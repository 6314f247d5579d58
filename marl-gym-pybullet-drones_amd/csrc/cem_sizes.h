// cem_sizes.h — host-side arithmetic of the CEM planner tick (qs_cem_*; plain C++,
// no HIP).
//
// A planner of horizon n over C candidates with K elites and I iterations on a
// handle with E envs of D drones and A action components owns nine device
// buffers.  As for the MPPI tick (planner_sizes.h, whose shape bounds it shares)
// three decisions are plain arithmetic and live here: how many bytes each buffer
// takes and whether the shape can be planned, which of the two select + refit
// variants runs, and the grids of the launches.
#pragma once

#include <cstddef>
#include <cstdint>

#include "planner_sizes.h"

namespace qs {

constexpr int kCemTag = 4;               // Philox domain tag of the CEM noise (3: the MPPI planner's)
constexpr int kCemThreads = kPlannerThreads;             // begin, sample, finish and the per-thread variants
constexpr int kCemBlockThreads = kPlannerBlockThreads;   // the per-workgroup select and refit
constexpr int kCemMaxElites = 1024;      // K at most: one elite per thread of the select workgroup
constexpr int kCemMaxIterations = 16;    // I at most (the counter word gives the iteration bits 8 .. 15)
constexpr int kCemStage = 4096;          // sort keys the per-workgroup select keeps in LDS (32 KB); the keys of
                                         // candidates beyond are formed again from ret / first_done at each pass

// The planner's buffers, in qs_cem_bufs' order.
enum { kCemMean = 0, kCemStd, kCemCandidates, kCemRet, kCemFirstDone, kCemElites, kCemIterBest, kCemAction, kCemTick,
       kCemBufs };

struct CemShape {
  int64_t n, C, K, I, E, D, A;
};

// Bytes of every buffer; false where the shape cannot be planned: whatever
// mppi_sizes refuses for (n, C, E, D, A) (horizon, candidate count, row width and
// the 32-bit offsets of qs_score), K outside 1 .. min(C, kCemMaxElites), or I
// outside 1 .. kCemMaxIterations.
inline bool cem_sizes(const CemShape& s, uint64_t b[kCemBufs]) {
  uint64_t m[kMppiBufs];
  if (!mppi_sizes(MppiShape{s.n, s.C, s.E, s.D, s.A}, m)) return false;
  if (s.K < 1 || s.K > s.C || s.K > kCemMaxElites) return false;
  if (s.I < 1 || s.I > kCemMaxIterations) return false;
  b[kCemMean] = m[kMppiNominal];
  b[kCemStd] = m[kMppiNominal];
  b[kCemCandidates] = m[kMppiCandidates];
  b[kCemRet] = m[kMppiRet];
  b[kCemFirstDone] = m[kMppiFirstDone];
  b[kCemElites] = (uint64_t)s.K * (uint64_t)s.E * 4u;   // K <= 1024, E < 2^31
  b[kCemIterBest] = (uint64_t)s.I * (uint64_t)s.E * 8u;
  b[kCemAction] = m[kMppiAction];
  b[kCemTick] = 8u;
  return true;
}

// Per-drone mode (qs_pd_cem_create): select and refit run over E · D "envs" with
// rows of A components (mppi_pd_shape).  The shape their variant and grids are taken from:
inline CemShape cem_pd_shape(const CemShape& s) { return CemShape{s.n, s.C, s.K, s.I, s.E * s.D, 1, s.A}; }
// Bytes of every buffer in per-drone mode and of the planner's ret_agent: elites
// grow to [K][E][D], iter_best to [I][E][D], the rest is cem_sizes'.  false where
// cem_sizes or mppi_pd_sizes refuses the shape.
inline bool cem_pd_sizes(const CemShape& s, uint64_t b[kCemBufs], uint64_t* ret_agent) {
  uint64_t m[kMppiBufs];
  if (!cem_sizes(s, b) || !mppi_pd_sizes(MppiShape{s.n, s.C, s.E, s.D, s.A}, m, ret_agent)) return false;
  const uint64_t agents = (uint64_t)s.E * (uint64_t)s.D;        // < 2^27 (mppi_pd_sizes)
  b[kCemElites] = (uint64_t)s.K * agents * 4u;                  // K <= 1024
  b[kCemIterBest] = (uint64_t)s.I * agents * 8u;                // I <= 16
  return true;
}

// Which select + refit runs.
//  kCemPerThread: select by one thread per env that ranks every candidate by
//    counting the candidates that come before it (C^2 comparisons a thread, reads
//    coalesced across the envs, no scratch); refit by one thread per (step, env,
//    drone, component) looping over the K elites.  Right for many envs and few
//    candidates.
//  kCemPerBlock: select by a workgroup per env (a radix select of the K-th
//    (score, candidate) key, C / 1024 keys a thread and pass, then the K elites
//    ranked among themselves); refit by a workgroup per (env, step) striding over
//    the elites, finishing with an in-wave tree and an LDS tree.
// The rule starts from mppi_variant's (C >= 64 and E · D · A < 256 CUs · 64 lanes)
// and adds one clause: from kCemBlockAlwaysC candidates on the workgroup variant
// runs whatever E is, since the per-thread count grows with C^2.
enum CemVariant { kCemPerThread = 0, kCemPerBlock = 1 };
constexpr int64_t kCemBlockAlwaysC = 512;
inline CemVariant cem_variant(int64_t E, int64_t C, int64_t row) {
  if (C >= kCemBlockAlwaysC) return kCemPerBlock;
  return mppi_variant(E, C, row) == kMppiPerBlock ? kCemPerBlock : kCemPerThread;
}

// Radix passes over the low word of the select key, C - 1 - c: its bytes up to
// the highest one that can be non-zero (1 .. 4; C <= 2^27).
inline int cem_index_bytes(int64_t C) {
  int nb = 1;
  while (nb < 4 && ((C - 1) >> (8 * nb)) != 0) ++nb;
  return nb;
}

// Grids (workgroups) of the launches.  All stay below 2^31 (C · E · D < 2^31,
// n <= 32 and a row of at most 256 components with E · row · 4 B · C below 2^31).
struct CemGrids {
  uint32_t fill;      // begin: kCemThreads threads, one per (j, e, d, a)
  uint32_t sample;    // x of a (sample, n) grid, kCemThreads threads each: one thread per (c, e, d) of a step
  uint32_t select;    // per thread: kCemThreads threads, one per env; per block: kCemBlockThreads, one workgroup per env
  uint32_t refit;     // per thread: kCemThreads threads, one per (j, e, d, a); per block: kCemBlockThreads, one per (e, j)
  uint32_t finish;    // kCemThreads threads, one per (e, d, a) column
};
inline CemGrids cem_grids(const CemShape& s, CemVariant v) {
  CemGrids g;
  const uint64_t col = (uint64_t)s.E * s.D * s.A;
  g.fill = mppi_div_up((uint64_t)s.n * col, kCemThreads);
  g.sample = mppi_div_up((uint64_t)s.C * s.E * s.D, kCemThreads);
  if (v == kCemPerBlock) {
    g.select = (uint32_t)s.E;
    g.refit = (uint32_t)(s.E * s.n);
  } else {
    g.select = mppi_div_up((uint64_t)s.E, kCemThreads);
    g.refit = g.fill;
  }
  g.finish = mppi_div_up(col, kCemThreads);
  return g;
}

}  // namespace qs
