// avoid_sizes.h — host-side arithmetic of the separation and obstacle terms (qs_avoid_score,
// qs_avoid_mppi_set / qs_avoid_cem_set; plain C++, no HIP).
//
// An avoidance spec names an obstacle table [M][8] float32 the score launch reads (centre,
// axis weights, radius, weight a row), and the radius, weight and height scale of the
// pairwise separation term.  What is plain arithmetic lives here: which specs are refused,
// the bytes of the table, which terms a launch sums at all, and whether cost_agent lies
// clear of a launch's other ranges.  The table's contents are device data: not read here.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace qs {

constexpr int kAvoidMaxRows = 16;      // M: rows of an obstacle table (the kernel's LDS copy, step_kernel.h kAvoidMaxObs)
constexpr int kAvoidRowFloats = 8;     // c[3], a[3], radius, weight
constexpr int kAvoidRowBytes = kAvoidRowFloats * 4;   // two 16-byte loads
constexpr int kAvoidAlign = 16;        // of `obstacles`

// Why an avoidance spec is refused (0: it is not).  The order is the order of the checks.
enum AvoidRefusal {
  kAvoidOk = 0,
  kAvoidRows,        // M outside 0 .. kAvoidMaxRows
  kAvoidTabNull,     // M > 0 and obstacles == NULL
  kAvoidTabAlign,    // M > 0 and obstacles not 16-byte aligned
  kAvoidRadius,      // sep_radius negative or not finite
  kAvoidWeight,      // sep_weight negative or not finite
  kAvoidZScale,      // sep_z_scale negative or not finite
};

// What of a qs_avoid_spec the checks read (the header's record stays out of this file).
struct AvoidSpecShape {
  uintptr_t obstacles;
  int64_t M;
  float sep_radius, sep_weight, sep_z_scale;
};

// A radius, weight or scale: finite and >= 0.  -0.0 is 0; a NaN fails the comparison.
inline bool avoid_number_ok(float v) { return v >= 0.0f && std::isfinite(v); }

// Bytes of obstacles [M][8] f32 for an M the checks accept.
inline uint64_t avoid_table_bytes(int64_t M) { return (uint64_t)M * (uint64_t)kAvoidRowBytes; }

// The checks of an avoidance spec, in the order of AvoidRefusal.  An M of 0 reads no
// table: its pointer may be anything.
inline AvoidRefusal avoid_refusal(const AvoidSpecShape& s) {
  if (s.M < 0 || s.M > kAvoidMaxRows) return kAvoidRows;
  if (s.M > 0) {
    if (s.obstacles == 0) return kAvoidTabNull;
    if (s.obstacles % (uintptr_t)kAvoidAlign != 0) return kAvoidTabAlign;
  }
  if (!avoid_number_ok(s.sep_radius)) return kAvoidRadius;
  if (!avoid_number_ok(s.sep_weight)) return kAvoidWeight;
  if (!avoid_number_ok(s.sep_z_scale)) return kAvoidZScale;
  return kAvoidOk;
}

// The refusal as the message after the entry point's name (nullptr: none).
inline const char* avoid_refusal_text(AvoidRefusal r) {
  switch (r) {
    case kAvoidRows: return "M must be within 0 .. 16";
    case kAvoidTabNull: return "obstacles is null";
    case kAvoidTabAlign: return "obstacles must be 16-byte aligned";
    case kAvoidRadius: return "sep_radius must be finite and >= 0";
    case kAvoidWeight: return "sep_weight must be finite and >= 0";
    case kAvoidZScale: return "sep_z_scale must be finite and >= 0";
    default: return nullptr;
  }
}

// Which terms a launch sums (the kernel forms the same two switches): a term whose
// switch is off is skipped, not added as zero.
inline bool avoid_sep_on(float sep_radius, float sep_weight, int64_t D) {
  return sep_radius != 0.0f && sep_weight != 0.0f && D > 1;
}
inline bool avoid_obs_on(int64_t M) { return M > 0; }

// Whether [lo, lo + bytes) meets [lo2, hi2): cost_agent against an output or action range.
inline bool avoid_ranges_meet(uintptr_t lo, uint64_t bytes, uintptr_t lo2, uintptr_t hi2) {
  const uintptr_t hi = lo + (uintptr_t)bytes;
  return lo < hi2 && lo2 < hi;
}

}  // namespace qs
