// step_score.h — host-side arithmetic of a branch-rollout launch (qs_score; plain
// C++, no HIP).
//
// qs_score runs C candidate action sequences of n steps from the handle's state
// in one launch of the FUSE = 3 step kernel over C · E virtual envs and stores
// nothing to the handle.  qs_score keeps no state from one launch to the next,
// so nothing is cut into several launches: a call is refused where a launch
// could not hold it (a branch set carries the state between launches:
// qs_branch_advance, step_branch.h).  Three decisions are plain arithmetic and live here: how
// many steps a launch takes (the steps' action rows wait in LDS), how many
// bytes each output of the C · E virtual envs covers, and whether the buffers
// the caller named keep out of each other's way.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace qs {

constexpr int kScoreMaxSteps = 32;      // = kMaxFuse (step_kernel.h), checked in quadswarm.hip
constexpr int kScoreStepBytes = 256;    // = kSeqStepBytes (step_fuse.h): an action component's row, one wave
constexpr int kScoreStepOuts = 7;       // = kFuseOuts (step_fuse.h): the outputs of a step
constexpr int kScoreOuts = kScoreStepOuts + 2;   // … then ret and first_done, once per call

// Steps of one launch.  A workgroup's LDS is `fixed` (the kernel's static
// workspace and the allocation grain), the history image where the instance
// keeps one (`hist_image`, else 0), the obs stage (`stage`) and kScoreStepBytes ·
// act_dim bytes per step; all of it stays within `limit`.  At most
// kScoreMaxSteps; 0 where not even one step fits.
inline int score_depth(size_t limit, size_t fixed, size_t hist_image, size_t stage, int act_dim) {
  const size_t used = fixed + hist_image + stage;
  if (act_dim < 1 || used >= limit) return 0;
  const size_t k = (limit - used) / ((size_t)kScoreStepBytes * (size_t)act_dim);
  return k > (size_t)kScoreMaxSteps ? kScoreMaxSteps : (int)k;
}

// Bytes of each buffer of a call over C candidates of a handle with E envs of D
// drones: b[0 .. 6] the outputs of a step in qs_step_out's order, b[7] ret, b[8]
// first_done, *act an action buffer.  The kernel indexes agents with 32-bit
// integers and the launch's grid by virtual env, so the virtual agent count must
// stay below 2^31; false where it does not.  Whether a single buffer is too
// large is score_fits' question, asked for the buffers the call names only.
struct ScoreShape {
  int64_t C, E, D, O, A, real_bytes;
};
inline bool score_sizes(const ScoreShape& s, uint64_t b[kScoreOuts], uint64_t* act) {
  if (s.C < 1 || s.E < 1 || s.D < 1 || s.O < 1 || s.A < 1 || s.real_bytes < 1) return false;
  const uint64_t lim = uint64_t(1) << 31;
  const uint64_t V = (uint64_t)s.C * (uint64_t)s.E;   // C, E < 2^31: no overflow
  if (V >= lim) return false;
  const uint64_t N = V * (uint64_t)s.D;               // V < 2^31, D <= 64
  if (N >= lim) return false;
  const uint64_t row = (uint64_t)s.O * 4u;            // N · row < 2^31 · 2^33
  b[0] = N * row; b[1] = V * (uint64_t)s.real_bytes; b[2] = V; b[3] = V; b[4] = N * row; b[5] = N;
  b[6] = N * (uint64_t)s.A * 4u;
  b[7] = V * 8u; b[8] = V * 4u;
  *act = b[6];
  return true;
}
// Bytes of qs_score_agents' ret_agent, [C][E][D] doubles, of a shape score_sizes
// accepted (C · E · D < 2^31, so the product stays far inside 64 bits).
inline uint64_t score_agent_bytes(const ScoreShape& s) {
  return (uint64_t)s.C * (uint64_t)s.E * (uint64_t)s.D * 8u;
}
// A buffer the kernel may address: its byte offsets fit 32 bits with room to spare.
inline bool score_fits(uint64_t bytes) { return bytes < (uint64_t(1) << 31); }

// The buffers of one call: every output range against every other output range
// and against every action range (action ranges may overlap each other: nobody
// writes them).  Ranges that only touch do not overlap.
struct ScoreRange {
  uintptr_t lo, hi;   // [lo, hi)
  bool action;
};
constexpr int kScoreMaxRanges = kScoreMaxSteps * (kScoreStepOuts + 1) + 3;   // … ret, first_done and ret_agent
struct ScoreRanges {
  ScoreRange r[kScoreMaxRanges];
  int n = 0;
  // false: no room left (more ranges than a call of kScoreMaxSteps steps can name)
  bool add(const void* p, uint64_t bytes, bool action) {
    if (!p || bytes == 0) return true;
    if (n >= kScoreMaxRanges) return false;
    r[n].lo = (uintptr_t)p;
    r[n].hi = (uintptr_t)p + (uintptr_t)bytes;
    r[n].action = action;
    n += 1;
    return true;
  }
  // Sorted by start, a range overlaps an earlier one iff it starts below the
  // largest end seen so far: among the outputs for an action range, among all
  // ranges for an output range.
  bool overlap() {
    std::sort(r, r + n, [](const ScoreRange& a, const ScoreRange& b) { return a.lo < b.lo; });
    uintptr_t out_end = 0, act_end = 0;
    for (int i = 0; i < n; ++i) {
      if (r[i].lo < out_end) return true;
      if (!r[i].action && r[i].lo < act_end) return true;
      uintptr_t& end = r[i].action ? act_end : out_end;
      if (r[i].hi > end) end = r[i].hi;
    }
    return false;
  }
};

}  // namespace qs
