// track_sizes.h — host-side arithmetic of the tracking cost (qs_track_score, qs_track_fold,
// qs_track_mppi_set / qs_track_cem_set; plain C++, no HIP).
//
// A tracking spec names a reference [L][E][D][12] float32 the score launch reads, a row
// base per env, twelve state weights, the action weights, a factor on the last step's
// state part and the task reward's weight in the folded objective.  What is plain
// arithmetic lives here: which specs are refused, the bytes of the reference with the
// 32-bit-offset bound of the kernel's buffer loads, the bytes of cost_agent, the row a
// step reads and the grid of the fold launch.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace qs {

constexpr int kTrackState = 12;      // pos, rpy, vel, angv: obs[0:12]
constexpr int kTrackMaxAct = 4;      // r[]: the first A are used
constexpr int kTrackRowBytes = kTrackState * 4;   // a drone's reference row: three 16-byte loads
constexpr int kTrackAlign = 16;      // of `ref`
constexpr int kTrackFoldThreads = 256;

// Why a tracking spec is refused (0: it is not).  The order is the order of the checks.
enum TrackRefusal {
  kTrackOk = 0,
  kTrackRefNull,     // ref == NULL
  kTrackRefAlign,    // ref not 16-byte aligned
  kTrackRows,        // L < 1
  kTrackQ,           // some q[k] negative or not finite
  kTrackR,           // some r[a], a < A, negative or not finite
  kTrackTerminal,    // terminal negative or not finite
  kTrackScale,       // reward_scale not finite
  kTrackOffsets,     // L · E · D · 48 bytes at or past 2^31
};

// What of a qs_track_spec the checks read (the header's record stays out of this file).
struct TrackSpecShape {
  uintptr_t ref;
  int64_t L;
  float q[kTrackState], r[kTrackMaxAct], terminal, reward_scale;
};

// A weight: finite and >= 0.  -0.0 is 0; a NaN fails the comparison.
inline bool track_weight_ok(float w) { return w >= 0.0f && std::isfinite(w); }

// Bytes of ref [L][E][D][12] f32.  false where an axis is empty or the bytes are at or
// past 2^31 (the kernel's 32-bit buffer offsets).  Every product is formed in 64 bits
// from factors bounded first.
inline bool track_ref_bytes(int64_t L, int64_t E, int64_t D, uint64_t* bytes) {
  const uint64_t lim = uint64_t(1) << 31;
  if (L < 1 || E < 1 || D < 1) return false;
  if ((uint64_t)L >= lim || (uint64_t)E >= lim || (uint64_t)D >= lim) return false;
  const uint64_t rows = (uint64_t)L * (uint64_t)E;   // < 2^62
  if (rows >= lim) return false;
  const uint64_t agents = rows * (uint64_t)D;        // < 2^62
  if (agents >= lim) return false;
  const uint64_t b = agents * (uint64_t)kTrackRowBytes;   // < 2^37
  if (b >= lim) return false;
  *bytes = b;
  return true;
}

// Bytes of cost_agent [C][E][D] f64 of a shape the score launch accepts (C · E · D < 2^31).
inline uint64_t track_cost_bytes(int64_t C, int64_t E, int64_t D) {
  return (uint64_t)C * (uint64_t)E * (uint64_t)D * 8u;
}

// The row step j of an env reads: clamp(base + j, 0, L − 1), with no sum that could wrap
// (base is any int32, 0 <= j <= 31, L >= 1).  The kernel forms the same value.
inline int32_t track_row(int32_t base, int32_t j, int32_t L) {
  const int64_t row = (int64_t)base + (int64_t)j;
  return row < 0 ? 0 : (row > (int64_t)L - 1 ? L - 1 : (int32_t)row);
}

// The checks of a tracking spec against a handle of E envs, D drones and A action
// components, in the order of TrackRefusal.
inline TrackRefusal track_refusal(const TrackSpecShape& s, int64_t E, int64_t D, int64_t A) {
  if (s.ref == 0) return kTrackRefNull;
  if (s.ref % (uintptr_t)kTrackAlign != 0) return kTrackRefAlign;
  if (s.L < 1) return kTrackRows;
  for (int k = 0; k < kTrackState; ++k)
    if (!track_weight_ok(s.q[k])) return kTrackQ;
  for (int a = 0; a < kTrackMaxAct && a < A; ++a)
    if (!track_weight_ok(s.r[a])) return kTrackR;
  if (!track_weight_ok(s.terminal)) return kTrackTerminal;
  if (!std::isfinite(s.reward_scale)) return kTrackScale;
  uint64_t bytes;
  if (!track_ref_bytes(s.L, E, D, &bytes)) return kTrackOffsets;
  return kTrackOk;
}

// Grid of the fold launch, kTrackFoldThreads threads a workgroup: one thread per (c, e).
// 0 where C · E is empty or at or past 2^31.
inline uint32_t track_fold_grid(int64_t C, int64_t E) {
  if (C < 1 || E < 1 || (uint64_t)C >= (uint64_t(1) << 31) || (uint64_t)E >= (uint64_t(1) << 31)) return 0;
  const uint64_t V = (uint64_t)C * (uint64_t)E;
  if (V >= (uint64_t(1) << 31)) return 0;
  return (uint32_t)((V + kTrackFoldThreads - 1) / kTrackFoldThreads);
}

}  // namespace qs
